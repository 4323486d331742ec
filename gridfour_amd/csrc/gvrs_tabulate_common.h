// gvrs_tabulate_common.h -- what the reference's data assessment computes per cell, restated once for host and device: the dense
// counters of InputDataStatCollector (demo/src/main/java/org/gridfour/demo/globalDEM/InputDataStatCollector.java:55-85) with the
// zMin / zMax / zSum that PackageData keeps beside them (PackageData.java:445-448, :504-533), and the symbol of a cell as
// EntropyTabulator counts it (demo/src/main/java/org/gridfour/demo/entropy/EntropyTabulator.java:227-246).  Used by the kernels of
// gvrs_tabulate.hip, by the C ABI (gvrs_api_tabulate.hip) and by a stand-alone CPU harness (tests/csrc/tabulate_harness.cpp).
//
// THE ARITHMETIC IS THE CONTRACT: results are compared bit for bit.  Everything here is integers, or FP64 with one rounding per
// operation (no fma: the build passes -ffp-contract=off), or a comparison with a definite tie rule.
#pragma once

#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "gvrs_common.h"

// ---- thresholds (tests/tabulate_cases.py reads these by text, so that its cases straddle them) ----
#define GF_TAB_THREADS 512             /* lanes of a workgroup of k_tabulate_dense (1024 would cap a lane at 64 VGPRs: spills)         */
#define GF_TAB_MAX_GROUPS 512          /* persistent workgroups of k_tabulate_dense at most: two per CU; the context's partials array  */
#define GF_TAB_LDS_MAX_BINS 36864      /* n_bins up to here: counters private to the workgroup in LDS (144 KiB); above: global atomics */
#define GF_TAB_SORT_THREADS 256        /* lanes of a workgroup of k_tab_digit_hist / k_tab_scatter: keys of one round                  */
#define GF_TAB_SORT_SHARE_MAX 4096     /* keys of a sort workgroup at most (a multiple of GF_TAB_SORT_THREADS) ...                     */
#define GF_TAB_SORT_SPREAD 2048        /* ... fewer while that keeps the workgroup count at or below this                              */
#define GF_TAB_SCAN_BLOCK 1024         /* entries of a workgroup of k_tab_digit_scan (phases 0 and 2); phase 1 takes 256 sums a trip   */
#define GF_TAB_RUN_BLOCK 2048          /* keys of a workgroup of k_tab_runs                                                            */
/* cells of one dense call above this: GF_ERR_UNSUPPORTED.  A lane numbers its own cells in an int32, so trips * cells-per-load must stay
 * below 2^31 (tabDense checks exactly that); with the full grid of 512 x 512 lanes that is reached near 2^49 cells.  2^40 is a round
 * bound far below it, and far above what device memory holds (2^40 SHORT cells are 2 TiB). */
#define GF_TAB_MAX_CELLS (1LL << 40)
#define GF_TAB_MAX_BINS (1 << 28)      /* n_bins above this: GF_ERR_UNSUPPORTED                                                        */

// Java's (int) of a double: truncating, saturating, NaN -> 0 (JLS 5.1.3)
GF_HD int32_t gf_tab_java_int(double x)
{
    if (x != x) return 0;
    if (x >= 2147483647.0) return 2147483647;
    if (x <= -2147483648.0) return (int32_t)(-2147483647 - 1);
    return (int32_t)x;
}

// the constructor's arithmetic: nCounter = (int)((defMax - defMin + 1) * scale) with the difference a Java int, base = (int)(defMin * scale),
// and the scale the samples see, which went through a float
struct GfTabPlan {
    int32_t nCounter, base;
    double scaleUsed;
};
GF_HD GfTabPlan gf_tab_plan(int32_t defMin, int32_t defMax, double scale)
{
    GfTabPlan p;
    const int32_t span = (int32_t)((uint32_t)defMax - (uint32_t)defMin + 1u);
    p.nCounter = gf_tab_java_int((double)span * scale);
    p.base = gf_tab_java_int((double)defMin * scale);
    p.scaleUsed = (double)(float)scale;
    return p;
}

// addSample's integer part: the sample of a value that is no NaN, and its counter (or -1: it touches none)
GF_HD int32_t gf_tab_sample(double v, double scaleUsed) { return gf_tab_java_int(v * scaleUsed + 0.5); }
// ... of an INT / SHORT cell where scale_used is exactly 1.0, without the FP64: v + 0.5 is exact, and the cast truncates toward zero,
// so v >= 0 gives v and v < 0 gives v + 1 (-3 + 0.5 = -2.5 -> -2; -2^31 + 0.5 -> -2^31 + 1); no int cell reaches the cast's limits
GF_HD int32_t gf_tab_sample_unit(int32_t v) { return (int32_t)((uint32_t)v + ((uint32_t)v >> 31)); }
GF_HD int32_t gf_tab_index(int32_t sample, int32_t base, int32_t nCounter)
{
    const uint32_t index = (uint32_t)sample - (uint32_t)base;
    return index > (uint32_t)nCounter ? -1 : (int32_t)index;              // (n_counter >= 0: one comparison is `index < 0 || index > nCounter`)
}

// EntropyTabulator's symbol of a cell: the int (a SHORT sign-extended), a float's raw bits
GF_HD uint32_t gf_tab_symbol_i32(int32_t v) { return (uint32_t)v; }
GF_HD uint32_t gf_tab_symbol_i16(int16_t v) { return (uint32_t)(int32_t)v; }

// zMin / zMax with the cell that holds them: `if (v < zMin) zMin = v` over the cells in row-major order keeps the FIRST cell that
// compares equal to the extreme, so of two candidates the one with the smaller value wins and, of equals (+0.0 and -0.0 are
// equal), the one with the smaller index.  at < 0: no candidate.  No NaN ever gets here.
template <typename T, typename AT = int64_t>
struct GfTabExt {
    T v;
    AT at;                         // int64: the cell's global index; the kernels' lanes count their own cells in an int32
};
template <typename T>
GF_HD bool gf_tab_min_better(const GfTabExt<T> &a, const GfTabExt<T> &b)      // a replaces b
{
    if (a.at < 0) return false;
    if (b.at < 0) return true;
    return a.v < b.v || (a.v == b.v && a.at < b.at);
}
template <typename T>
GF_HD bool gf_tab_max_better(const GfTabExt<T> &a, const GfTabExt<T> &b)
{
    if (a.at < 0) return false;
    if (b.at < 0) return true;
    return a.v > b.v || (a.v == b.v && a.at < b.at);
}

// what one part of a block adds up to: a lane's, a wave's, a workgroup's cells (all sums wrap as Java longs do)
template <typename T, typename AT = int64_t>
struct GfTabPart {
    uint64_t nSkipped, nSamples, sumSamples, sumI;
    GfTabExt<T, AT> mn, mx;
};
template <typename T, typename AT>
GF_HD void gf_tab_part_start(GfTabPart<T, AT> &p)
{
    p.nSkipped = p.nSamples = p.sumSamples = p.sumI = 0;
    p.mn.v = p.mx.v = T(0);
    p.mn.at = p.mx.at = -1;
}
template <typename T>
GF_HD void gf_tab_part_merge(GfTabPart<T> &p, const GfTabPart<T> &q)
{
    p.nSkipped += q.nSkipped, p.nSamples += q.nSamples, p.sumSamples += q.sumSamples, p.sumI += q.sumI;
    if (gf_tab_min_better(q.mn, p.mn)) p.mn = q.mn;
    if (gf_tab_max_better(q.mx, p.mx)) p.mx = q.mx;
}

// the call's constants as the kernels and the harness take them
struct GfTabDenseGeom {
    int64_t nCells, firstCell;
    double scaleUsed;
    int32_t base, nCounter;
    int32_t elemType;              // GF_ELEM_*: 0 INT, 1 SHORT, 2 FLOAT
    int32_t fillI, skipFill;
    int32_t pad_;
};

// One cell, visited in ascending order of `at` by whoever owns p (so a strict comparison keeps the first of equals).  Returns the
// counter to increment, or -1.  UNIT: the cell is an int and g.scaleUsed is 1.0 (gf_tab_sample_unit).
template <bool UNIT = false, typename T, typename AT>
GF_HD int32_t gf_tab_cell(const GfTabDenseGeom &g, T cell, AT at, GfTabPart<T, AT> &p)
{
    bool isSample;
    if constexpr (std::is_floating_point_v<T>) isSample = cell == cell;                         // FLOAT: a NaN is no sample
    else isSample = !(g.skipFill && (int32_t)cell == g.fillI);
    if (!isSample) {
        p.nSkipped++;
        return -1;
    }
    if (p.mn.at < 0 || cell < p.mn.v) p.mn.v = cell, p.mn.at = at;
    if (p.mx.at < 0 || cell > p.mx.v) p.mx.v = cell, p.mx.at = at;
    if constexpr (!std::is_floating_point_v<T>) p.sumI += (uint64_t)(int64_t)cell;
    int32_t sample;
    if constexpr (UNIT) sample = gf_tab_sample_unit((int32_t)cell);
    else sample = gf_tab_sample((double)cell, g.scaleUsed);
    const int32_t index = gf_tab_index(sample, g.base, g.nCounter);
    if (index >= 0) {
        p.nSamples++;
        p.sumSamples += (uint64_t)(int64_t)sample;
    }
    return index;
}

// keys of a workgroup of the sort: few enough workgroups for the histograms to stay small, enough of them to fill the chip on a
// modest block
GF_HD uint32_t gf_tab_sort_share(uint32_t n)
{
    const uint32_t per = (n + GF_TAB_SORT_SPREAD - 1u) / GF_TAB_SORT_SPREAD;
    const uint32_t share = (per + GF_TAB_SORT_THREADS - 1u) / GF_TAB_SORT_THREADS * GF_TAB_SORT_THREADS;
    return share < GF_TAB_SORT_THREADS ? GF_TAB_SORT_THREADS : share > GF_TAB_SORT_SHARE_MAX ? GF_TAB_SORT_SHARE_MAX : share;
}

// gf_tab_summary / gf_tab_symbols of include/gvrs_hip_codec.h as the kernels write them
struct GfTabSummary {
    int64_t nCells, nSkipped, nSamples, sumSamples, sumI;
    double mn, mx;
    int64_t mnAt, mxAt;
};
// the summary of a call from the merged part of its cells; accumulate: merged with what the summary held
GF_HD void gf_tab_finish(GfTabSummary &s, GfTabPart<double> d, int accumulate, int64_t nCells)
{
    int64_t cells = nCells;
    if (accumulate) {
        GfTabPart<double> old;
        old.nSkipped = (uint64_t)s.nSkipped, old.nSamples = (uint64_t)s.nSamples, old.sumSamples = (uint64_t)s.sumSamples, old.sumI = (uint64_t)s.sumI;
        old.mn.v = s.mn, old.mn.at = s.mnAt, old.mx.v = s.mx, old.mx.at = s.mxAt;
        gf_tab_part_merge(old, d);
        d = old;
        cells = (int64_t)((uint64_t)s.nCells + (uint64_t)nCells);
    }
    s.nCells = cells;
    s.nSkipped = (int64_t)d.nSkipped, s.nSamples = (int64_t)d.nSamples, s.sumSamples = (int64_t)d.sumSamples, s.sumI = (int64_t)d.sumI;
    s.mn = d.mn.at < 0 ? (double)INFINITY : d.mn.v, s.mnAt = d.mn.at < 0 ? -1 : d.mn.at;
    s.mx = d.mx.at < 0 ? -(double)INFINITY : d.mx.v, s.mxAt = d.mx.at < 0 ? -1 : d.mx.at;
}
template <typename T>
GF_HD GfTabPart<double> gf_tab_widen(const GfTabPart<T> &p)
{
    GfTabPart<double> d;
    d.nSkipped = p.nSkipped, d.nSamples = p.nSamples, d.sumSamples = p.sumSamples, d.sumI = p.sumI;
    d.mn.v = (double)p.mn.v, d.mn.at = p.mn.at, d.mx.v = (double)p.mx.v, d.mx.at = p.mx.at;            // (exact for every type)
    return d;
}
struct GfTabSymbols {
    int64_t nSamples, nSymbols, nUnique, nRepeated, nWritten;
    int32_t maxCount, reserved;
};
