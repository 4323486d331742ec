// gvrs_downsample_common.h -- the box average of the reference's ExampleDownsample, restated once for host and device: what one
// output cell is, given the f x f window of source cells in row-major order
// (demo/src/main/java/org/gridfour/demo/globalDEM/ExampleDownsample.java:185-206).  Used by the kernels of gvrs_downsample.hip
// and by a stand-alone CPU harness (tests/csrc/downsample_harness.cpp).
//
// THE ARITHMETIC IS THE CONTRACT: results are compared bit for bit.
//   INT, SHORT (and the codes of an int-coded float): a window with ANY cell equal to the fill gives the fill; else the cells are
//   summed as Java ints (wrap-around), avg = (double) sum / n is one IEEE double division, the result (int) Math.floor(avg + 0.5).
//   |avg| <= 2^31, so the cast never saturates; a SHORT's result fits int16 also after a wrapped sum (2^31 / n < 32768 once the
//   sum of n int16 can wrap).
//   FLOAT: float sum = 0; sum += cell for every cell IN ORDER, one float32 rounding per addition; the result sum / (float) n, one
//   correctly rounded float32 division.  The fill is not looked at.  No wider accumulator, no reassociation, no fma (the build
//   passes -ffp-contract=off), no flushing of subnormals: 0.0f + -0.0f is +0.0f, inf + -inf is NaN.
// n = f * f <= 46340^2 fits Java's int.
#pragma once

#include <math.h>
#include <stdint.h>

#include "gvrs_common.h"

// the integer window: the wrapped sum and "a fill was seen".  The sum is associative and the fill test an OR, so parts of a window
// may be accumulated apart and merged; the float chain below may not.
struct GfDsIntAcc {
    uint32_t sum;
    uint32_t fillSeen;
};

GF_HD void gf_ds_int_start(GfDsIntAcc &a) { a.sum = 0, a.fillSeen = 0; }

GF_HD void gf_ds_int_add(GfDsIntAcc &a, int32_t cell, int32_t fill)
{
    a.fillSeen |= (uint32_t)(cell == fill);
    a.sum += (uint32_t)cell;                                   // Java's int +=
}

GF_HD int32_t gf_ds_int_finish(const GfDsIntAcc &a, int32_t fill, int32_t n)
{
    if (a.fillSeen) return fill;                               // the output cell is left unpopulated
    const double avg = (double)(int32_t)a.sum / (double)n;
    return (int32_t)floor(avg + 0.5);
}

GF_HD void gf_ds_float_start(float &sum) { sum = 0.0f; }

GF_HD void gf_ds_float_add(float &sum, float cell) { sum = sum + cell; }

GF_HD float gf_ds_float_finish(float sum, int32_t n) { return sum / (float)n; }

// The geometry of one call, as the kernels and the harness take it.  The block holds pitch cells per row; output cell (i, j) of
// outRows x outCols averages block rows rowOff + i * f .. + f - 1 and columns colOff + j * f .. + f - 1.
#define GF_DS_ARGB 3
struct GfDsGeom {
    int64_t pitch;                 // cells per block row (the block's n_cols)
    int64_t outRows, outCols;
    int32_t rowOff, colOff;        // the first window's corner inside the block, each in 0 .. f - 1
    int32_t f;                     // the factor, 1 .. 46340
    int32_t elemType;              // GF_ELEM_*: 0 INT, 1 SHORT, 2 FLOAT; GF_DS_ARGB: packed ARGB words (gvrs_image_common.h; fillI unused)
    int32_t fillI;
};

// gf_block_downsample_rect's rule for one axis: the coarse cells whose whole window lies in [at, at + n)
GF_HD void gf_ds_axis(int32_t at, int32_t n, int32_t f, int32_t &outAt, int32_t &outN)
{
    const int64_t first = ((int64_t)at + f - 1) / f, end = ((int64_t)at + n) / f;
    outAt = (int32_t)first;
    outN = end > first ? (int32_t)(end - first) : 0;
}

// one output cell from the block, cell by cell: the harness' whole route, and what every kernel path must equal
GF_HD int32_t gf_ds_cell_int32(const GfDsGeom &g, const int32_t *block, int64_t i, int64_t j)
{
    GfDsIntAcc a;
    gf_ds_int_start(a);
    const int32_t *p = block + ((int64_t)g.rowOff + i * g.f) * g.pitch + g.colOff + j * g.f;
    for (int32_t r = 0; r < g.f; r++, p += g.pitch)
        for (int32_t c = 0; c < g.f; c++) gf_ds_int_add(a, p[c], g.fillI);
    return gf_ds_int_finish(a, g.fillI, g.f * g.f);
}

GF_HD int16_t gf_ds_cell_int16(const GfDsGeom &g, const int16_t *block, int64_t i, int64_t j)
{
    GfDsIntAcc a;
    gf_ds_int_start(a);
    const int16_t *p = block + ((int64_t)g.rowOff + i * g.f) * g.pitch + g.colOff + j * g.f;
    for (int32_t r = 0; r < g.f; r++, p += g.pitch)
        for (int32_t c = 0; c < g.f; c++) gf_ds_int_add(a, p[c], g.fillI);
    return (int16_t)gf_ds_int_finish(a, g.fillI, g.f * g.f);
}

GF_HD float gf_ds_cell_float(const GfDsGeom &g, const float *block, int64_t i, int64_t j)
{
    float sum;
    gf_ds_float_start(sum);
    const float *p = block + ((int64_t)g.rowOff + i * g.f) * g.pitch + g.colOff + j * g.f;
    for (int32_t r = 0; r < g.f; r++, p += g.pitch)
        for (int32_t c = 0; c < g.f; c++) gf_ds_float_add(sum, p[c]);
    return gf_ds_float_finish(sum, g.f * g.f);
}
