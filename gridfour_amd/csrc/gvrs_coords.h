// gvrs_coords.h -- the coordinate rules of a GVRS file, restated once for host and device: how geographic and model coordinates
// map to grid coordinates and back (gvrs/GvrsFileSpecification.java:2101-2105 mapGridToModelPoint, :2122-2126 mapModelToGridPoint,
// :2159-2173 mapGeographicToGridPoint, :2198-2212 makeGridPointUsingFringe, :2230-2234 mapGridToGeoPoint; util/Angle.java:57-85
// to180 / to360), what the reference derives from a file when it opens one (:695-707 checkGeographicCoverage, :435-440 the
// fringes; gvrs/GvrsInterpolatorBSpline.java:120-131 du and dv) and the column spacing of zNormal / zNormalGrid (:226-232,
// :291-299).  Used by k_coords_map (gvrs_coords.hip), by the coordinate instantiations of k_points_mark and k_points_interp
// (gvrs_file_points.hip), by the host forms (gvrs_api_coords.hip, gvrs_api_file_points.hip) and by a stand-alone CPU program
// (tests/csrc/coords_test.cpp).
//
// THE ARITHMETIC IS THE CONTRACT, as in gvrs_interp_common.h: doubles, the reference's operands, order and association, one
// rounding per operation (built with -ffp-contract=off; no fma()).  Java's % on doubles is fmod.
//
// toRadians(a) = a * 0.017453292519943295: Math.toRadians of JDK 9 and later (DEGREES_TO_RADIANS).  JDK 8 computed
// a / 180.0 * PI, which differs in the last bit for some arguments; the later one was chosen.
//
// TWO DELIBERATE DEVIATIONS from the reference:
//   1. THE COSINE is gf_strict_cos: StrictMath.cos's value, fdlibm 5.3's algorithm, which is specified exactly.  The reference
//      calls Math.cos, which is only specified to within 1 ulp and is PERMITTED to return exactly StrictMath.cos; on a JVM whose
//      intrinsic differs, the spacing here differs from the reference's by that ulp for some latitudes.  A caller who needs
//      another cosine passes per-point column spacings.
//   2. THE LATITUDE CHECK: z() refuses |y| > 90.0001 by throwing (GvrsInterpolatorBSpline.java:169-172), zNormal() omits the
//      check.  Here a query of a geographic file whose latitude has |lat| > 90.0001 is refused (GF_IP_ERR_ARG) at every target;
//      NaN passes, as in Java, and is refused later by the window.  This keeps the cosine's argument inside |x| < 3 pi / 4, the
//      range gf_strict_cos is written for.
// Reference paths are relative to core/src/main/java/org/gridfour/.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "gvrs_common.h"
#include "gvrs_interp_common.h"

// how the points of a fused call are given (GF_COORDS_* of include/gvrs_hip_codec.h)
#define GF_CO_GRID 0
#define GF_CO_FILE 1
// the mappings (GF_MAP_* of include/gvrs_hip_codec.h)
#define GF_CO_GEO_TO_GRID 0
#define GF_CO_MODEL_TO_GRID 1
#define GF_CO_GRID_TO_GEO 2
#define GF_CO_GRID_TO_MODEL 3

// what the rules read of a file: the header's facts and what the reference derives from them when it opens the file
struct GfCoords {
    int32_t nRowsGrid, nColsGrid;
    int32_t geographic;                             // isGeographicCoordinateSystemSpecified: coordinate_system == 2
    int32_t wrap;                                   // 0; 1 geoWrapsLongitude; 2 geoBracketsLongitude
    double x0, y0, x1, y1, cellSizeX, cellSizeY;
    double m2r[6], r2m[6];                          // 00 01 02 10 11 12, the file's order
    double rowFringe0, rowFringe1, colFringe0, colFringe1;
    double du, dv;                                  // GvrsInterpolatorBSpline's
};

// ---- bits of a double ----
GF_HD int32_t gf_coords_hi(double x)                                           // fdlibm's __HI
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2hiint(x);
#else
    uint64_t u;
    memcpy(&u, &x, 8);
    return (int32_t)(u >> 32);
#endif
}
GF_HD double gf_coords_of_bits(uint64_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)u);
#else
    double x;
    memcpy(&x, &u, 8);
    return x;
#endif
}
GF_HD uint64_t gf_coords_bits(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__double_as_longlong(x);
#else
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
#endif
}
// Math.ulp of a finite x: the distance to the next double of larger magnitude
GF_HD double gf_coords_ulp(double x)
{
    const double a = fabs(x);
    return gf_coords_of_bits(gf_coords_bits(a) + 1u) - a;
}

// ---- util/Angle.java ----
// :57-67
GF_HD double gf_coords_to180(double angle)
{
    const double a = fmod(angle, 360.0);
    if (a == 0) return 0;                                                      // (avoid -0)
    else if (a < -180) return 360 + a;
    else if (a >= 180) return a - 360;
    return a;
}
// :76-85
GF_HD double gf_coords_to360(double angle)
{
    const double a = fmod(angle, 360.0);
    if (a < 0) return a + 360;
    else if (a == 0) return 0;
    else return a;
}

GF_HD double gf_coords_radians(double a) { return a * 0.017453292519943295; }

// ---- StrictMath.cos for |x| < 3 pi / 4: fdlibm 5.3 (k_cos.c, k_sin.c, the n = +-1 branch of e_rem_pio2.c, s_cos.c) ----
// __kernel_cos(x, y): cos(x + y) for |x| <= pi / 4, y the tail of x
GF_HD double gf_coords_kernel_cos(double x, double y)
{
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05;
    const double C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const int32_t ix = gf_coords_hi(x) & 0x7fffffff;
    if (ix < 0x3e400000) return 1.0;                                           // |x| < 2^-27: (int) x == 0 always
    const double z = x * x;
    const double r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    if (ix < 0x3FD33333) return 1.0 - (0.5 * z - (z * r - x * y));             // |x| < 0.3
    double qx;
    if (ix > 0x3fe90000) qx = 0.28125;                                         // x > 0.78125
    else qx = gf_coords_of_bits((uint64_t)(uint32_t)(ix - 0x00200000) << 32);  // x / 4, from the high word alone
    const double hz = 0.5 * z - qx;
    const double a = 1.0 - qx;
    return a - (hz - (z * r - x * y));
}
// __kernel_sin(x, y, 1): sin(x + y) for |x| <= pi / 4, y the tail of x
GF_HD double gf_coords_kernel_sin(double x, double y)
{
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04;
    const double S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const int32_t ix = gf_coords_hi(x) & 0x7fffffff;
    if (ix < 0x3e400000) return x;                                             // |x| < 2^-27
    const double z = x * x;
    const double v = z * x;
    const double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
// cos(x); NaN for a NaN or infinite x and OUTSIDE |x| < 3 pi / 4 (fdlibm goes on into rem_pio2's other branches there, which
// are not restated: the latitude check keeps every caller inside)
GF_HD double gf_strict_cos(double x)
{
    const double pio2_1 = 1.57079632673412561417e+00, pio2_1t = 6.07710050650619224932e-11;
    const double pio2_2 = 6.07710050630396597660e-11, pio2_2t = 2.02226624879595063154e-21;
    const int32_t hx = gf_coords_hi(x), ix = hx & 0x7fffffff;
    if (ix <= 0x3fe921fb) return gf_coords_kernel_cos(x, 0.0);                 // |x| <= pi / 4
    if (ix >= 0x4002d97c) return gf_coords_of_bits(0x7ff8000000000000ull);
    double y0, y1;
    if (hx > 0) {                                                              // n = 1: cos x = -sin(x - pi / 2)
        double z = x - pio2_1;
        if (ix != 0x3ff921fb) {                                                // 33 + 53 bits of pi are good enough
            y0 = z - pio2_1t;
            y1 = (z - y0) - pio2_1t;
        } else {                                                               // near pi / 2: 33 + 33 + 53 bits
            z -= pio2_2;
            y0 = z - pio2_2t;
            y1 = (z - y0) - pio2_2t;
        }
        return -gf_coords_kernel_sin(y0, y1);
    }
    double z = x + pio2_1;                                                     // n = -1: cos x = sin(x + pi / 2)
    if (ix != 0x3ff921fb) {
        y0 = z + pio2_1t;
        y1 = (z - y0) + pio2_1t;
    } else {
        z += pio2_2;
        y0 = z + pio2_2t;
        y1 = (z - y0) + pio2_2t;
    }
    return gf_coords_kernel_sin(y0, y1);
}

// ---- what the reference derives when it opens a file: fills nRowsGrid .. r2m from the arguments, then wrap, fringes, du, dv ----
GF_HD void gf_coords_derive(GfCoords &c)
{
    c.wrap = 0;
    if (c.geographic) {                                                        // checkGeographicCoverage (:695-707)
        const double gxDelta = c.x1 - c.x0;
        if (gxDelta == 360) c.wrap = 2;
        else {
            const double a360 = fabs(gf_coords_to180(c.x1 + c.cellSizeX - c.x0));
            c.wrap = a360 < 1.0e-6 ? 1 : 0;
        }
    }
    const double xUlp = gf_coords_ulp((double)c.nColsGrid), yUlp = gf_coords_ulp((double)c.nRowsGrid);   // (:435-440)
    c.colFringe0 = -0.5 - 4 * xUlp;
    c.colFringe1 = c.nColsGrid - 0.5 + 4 * xUlp;
    c.rowFringe0 = -0.5 - 4 * yUlp;
    c.rowFringe1 = c.nRowsGrid - 0.5 + 4 * yUlp;
    const double rEarth = 6371007.2;                                           // (GvrsInterpolatorBSpline.java:99, :120-131)
    if (c.geographic) {
        c.du = rEarth * gf_coords_radians(c.cellSizeX);
        c.dv = rEarth * gf_coords_radians(c.cellSizeY);
    } else {
        c.du = c.cellSizeX;
        c.dv = c.cellSizeY;
    }
}

// ---- the mappings ----
// mapGeographicToGridPoint (:2159-2171), without its GridPoint
GF_HD void gf_coords_geo_to_grid(const GfCoords &c, double latitude, double longitude, double &row, double &col)
{
    row = (latitude - c.y0) / c.cellSizeY;
    const double delta = longitude - c.x0;
    col = delta / c.cellSizeX;
    if (col < c.colFringe0 || col > c.colFringe1) {
        col = gf_coords_to180(delta) / c.cellSizeX;
        if (col < c.colFringe0 || col > c.colFringe1) col = gf_coords_to360(delta) / c.cellSizeX;
    }
}
// mapModelToGridPoint (:2122-2124)
GF_HD void gf_coords_model_to_grid(const GfCoords &c, double x, double y, double &row, double &col)
{
    col = x * c.m2r[0] + y * c.m2r[1] + c.m2r[2];
    row = x * c.m2r[3] + y * c.m2r[4] + c.m2r[5];
}
// makeGridPointUsingFringe (:2198-2212): the GridPoint's integer row and column
GF_HD void gf_coords_grid_point(const GfCoords &c, double row, double col, int32_t &iRowOut, int32_t &iColOut)
{
    int32_t iRow = gf_interp_java_int(floor(row + 0.5));
    int32_t iCol = gf_interp_java_int(floor(col + .5));
    if (iRow == -1 && row >= c.rowFringe0) iRow = 0;
    else if (iRow >= c.nRowsGrid && row <= c.rowFringe1) iRow = c.nRowsGrid - 1;
    if (iCol == -1 && col >= c.colFringe0) iCol = 0;
    else if (iCol >= c.nColsGrid && col <= c.colFringe1) iCol = c.nColsGrid - 1;
    iRowOut = iRow, iColOut = iCol;
}
// mapGridToGeoPoint (:2230-2234)
GF_HD void gf_coords_grid_to_geo(const GfCoords &c, double row, double col, double &lat, double &lon)
{
    lat = (c.y1 - c.y0) * row / (c.nRowsGrid - 1) + c.y0;
    lon = (c.x1 - c.x0) * col / (c.nColsGrid - 1) + c.x0;
}
// mapGridToModelPoint (:2101-2105)
GF_HD void gf_coords_grid_to_model(const GfCoords &c, double row, double col, double &x, double &y)
{
    x = col * c.r2m[0] + row * c.r2m[1] + c.r2m[2];
    y = col * c.r2m[3] + row * c.r2m[4] + c.r2m[5];
}

// ---- the interpolator's rules ----
// z()'s check (GvrsInterpolatorBSpline.java:169); a NaN passes
GF_HD bool gf_coords_lat_refused(const GfCoords &c, double lat) { return c.geographic && fabs(lat) > 90.0001; }
// the column spacing of zNormal (:226-232) and zNormalGrid (:291-299) at latitude lat, du the interpolator's
GF_HD double gf_coords_col_spacing(const GfCoords &c, double du, double lat)
{
    if (!c.geographic) return du;
    const double s = gf_strict_cos(gf_coords_radians(lat));
    double dx = s * du;
    if (dx < 1) dx = 1;
    return dx;
}

// A query point of a fused call, the one function k_points_mark, k_points_interp and the host's bitmap share: (a, b) given as
// kind says -- GF_CO_GRID: (row, column); GF_CO_FILE: (x, y) as z() / zNormal() read them -- to the grid coordinates the window
// takes and the column spacing of the rule (du: the interpolator's column spacing; withSpacing false: du itself, for a caller
// that has no use for the spacing or brings its own).  GF_IP_ERR_ARG, with NaN for all three, where the latitude check refuses:
// the latitude is y, or mapGridToGeoPoint's for a point in grid coordinates.
struct GfCoordsQuery {
    double row, col, spacing;
};
GF_HD int gf_coords_query(const GfCoords &c, int kind, double a, double b, double du, bool withSpacing, GfCoordsQuery &q)
{
    double lat = 0, lon = 0;
    if (kind == GF_CO_GRID) {
        q.row = a, q.col = b;
        if (c.geographic) gf_coords_grid_to_geo(c, a, b, lat, lon);
    } else {
        lat = b;
        if (c.geographic) gf_coords_geo_to_grid(c, b, a, q.row, q.col);
        else gf_coords_model_to_grid(c, a, b, q.row, q.col);
    }
    if (gf_coords_lat_refused(c, lat)) {
        q.row = q.col = q.spacing = gf_coords_of_bits(0x7ff8000000000000ull);
        return GF_IP_ERR_ARG;
    }
    q.spacing = withSpacing ? gf_coords_col_spacing(c, du, lat) : du;
    return GF_IP_OK;
}

// One point of gf_file_map_points: (a, b) mapped as kind says.  To-grid kinds: (x, y) -> outA = row, outB = column, the
// GridPoint's integers, the column spacing of the rule with the file's du, and GF_IP_ERR_ARG (NaN, NaN, 0, 0, NaN) where the
// latitude check refuses y.  From-grid kinds: (row, column) -> outA = x (the longitude), outB = y (the latitude); the rest is
// left alone.  The geo kinds do not ask which system the file states, as the reference's mapping functions do not; the
// latitude check and the spacing ask the file, as the interpolator does.  A NaN result leaves as THE canonical NaN
// (0x7ff8000000000000, what Double.doubleToLongBits reports for every NaN): the sign and payload of a generated NaN are the
// machine's, not the rule's, and host and device forms are compared bit for bit.
GF_HD double gf_coords_canonical(double x) { return x != x ? gf_coords_of_bits(0x7ff8000000000000ull) : x; }
struct GfCoordsMapped {
    double outA, outB, spacing;
    int32_t iRow, iCol, status;
};
GF_HD void gf_coords_map(const GfCoords &c, int kind, double a, double b, GfCoordsMapped &m)
{
    m.iRow = m.iCol = 0, m.status = GF_IP_OK, m.spacing = 0;
    if (kind == GF_CO_GRID_TO_GEO) gf_coords_grid_to_geo(c, a, b, m.outB, m.outA);
    else if (kind == GF_CO_GRID_TO_MODEL) gf_coords_grid_to_model(c, a, b, m.outA, m.outB);
    else {
        if (gf_coords_lat_refused(c, b)) {
            m.outA = m.outB = m.spacing = gf_coords_of_bits(0x7ff8000000000000ull);
            m.status = GF_IP_ERR_ARG;
            return;
        }
        if (kind == GF_CO_GEO_TO_GRID) gf_coords_geo_to_grid(c, b, a, m.outA, m.outB);
        else gf_coords_model_to_grid(c, a, b, m.outA, m.outB);
        gf_coords_grid_point(c, m.outA, m.outB, m.iRow, m.iCol);
        m.spacing = gf_coords_canonical(gf_coords_col_spacing(c, c.du, b));
    }
    m.outA = gf_coords_canonical(m.outA), m.outB = gf_coords_canonical(m.outB);
}
