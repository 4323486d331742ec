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
#define GF_TAB_MERGE_BLOCK 2048        /* positions of the merged sequence of a workgroup of k_tab_merge (GF_TAB_SORT_THREADS lanes)  */
#define GF_TAB_SHORT_MAX_GROUPS 256    /* persistent workgroups of k_tab_short_counts at most: its LDS window lets one live on a CU   */
#define GF_TAB_SHORT_WIN_LO (-16384)   /* SHORT cells from here ...                                                                    */
#define GF_TAB_SHORT_WIN_HI 16383      /* ... up to here count in the workgroup's LDS (128 KiB), the others by global atomics         */
#define GF_TAB_COMPACT_THREADS 1024    /* lanes of the one workgroup of k_tab_short_compact: 64 of the 65,536 counters each           */
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

// ---- the merge of two symbol tables (k_tab_merge of gvrs_tabulate.hip; tests/csrc/tabulate_merge_harness.cpp) ----
// A table: n symbols in strictly ascending unsigned order, each with an int32 count.  THE MERGED SEQUENCE of tables A and B is all
// nA + nB entries in ascending order, A's in front of B's where the symbols are equal: a symbol that both tables hold is a pair of
// neighbours, A's entry first, and since each table is strictly ascending nothing occurs more than twice.  THE PAIR RULE: an
// entry of the merged sequence is a HEAD iff it is the first one or its symbol differs from its predecessor's; a head's count is
// its own plus, where its successor holds the same symbol, the successor's, with int32 wrap (EntropyTabulator.java:239-240: the
// counter is a Java int).  The result is the heads in order.  A part of the merged sequence (a workgroup's chunk, a lane's run)
// therefore looks one entry back and one entry ahead and at nothing else: a part whose first entry repeats its predecessor drops
// it, a part whose last entry is repeated by its successor takes the successor's count.  Tables that are not strictly ascending
// give an unspecified result by the same rule: every index is checked against its table's length.

// the entries of a table that count: min(n_written, cap); none without a summary (or, for the accumulate form, without samples)
GF_HD uint32_t gf_tab_table_len(const GfTabSymbols *s, uint32_t cap, bool emptyWithoutSamples)
{
    if (!s || (emptyWithoutSamples && s->nSamples == 0)) return 0u;
    const int64_t w = s->nWritten;
    return w <= 0 ? 0u : w < (int64_t)cap ? (uint32_t)w : cap;
}

// THE SPLIT: how many of the first d entries of the merged sequence are A's (the other d - that are B's); d <= nA + nB
GF_HD uint32_t gf_tab_merge_split(const uint32_t *a, uint32_t nA, const uint32_t *b, uint32_t nB, uint64_t d)
{
    uint32_t lo = d > nB ? (uint32_t)(d - nB) : 0u, hi = d < nA ? (uint32_t)d : nA;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (a[mid] <= b[d - 1u - mid]) lo = mid + 1u;                      // A's entry stands in front of B's unless it is larger
        else hi = mid;
    }
    return lo;
}

// at the cursor (ia of A's entries and ib of B's are behind it): is the next entry A's?  (one of the tables has an entry left)
GF_HD bool gf_tab_merge_next_is_a(const uint32_t *a, uint32_t nA, const uint32_t *b, uint32_t nB, uint32_t ia, uint32_t ib)
{
    return ib >= nB || (ia < nA && a[ia] <= b[ib]);
}

// What a chunk [d0, d1) of the merged sequence needs of the tables, from the splits at d0 and at d1 (sa0, sa1: A's entries in
// front of them): A[a0, a1) and B[b0, b1) are the chunk's entries with the one entry of each table in front of the chunk and the
// one behind it, where there is one; `pre` of them (0, 1 or 2) stand in front of the chunk, and they are the first `pre` entries
// of the two windows' own merged sequence.  At most d1 - d0 + 4 entries.
struct GfTabMergeWindow {
    uint32_t a0, a1, b0, b1, pre;
};
GF_HD GfTabMergeWindow gf_tab_merge_window(uint32_t nA, uint32_t nB, uint64_t d0, uint32_t sa0, uint64_t d1, uint32_t sa1)
{
    // (tables that are not ascending may give splits that do not follow one another: sa1 is held to sa0 <= sa1 <= sa0 + (d1 - d0)
    // and to d1 - nB <= sa1 <= nA, which for ascending tables it meets anyway, so that both windows stay inside their tables)
    const uint64_t lo = d1 > nB && d1 - nB > sa0 ? d1 - nB : sa0, hi = sa0 + (d1 - d0) < nA ? sa0 + (d1 - d0) : nA;
    sa1 = sa1 < lo ? (uint32_t)lo : sa1 > hi ? (uint32_t)hi : sa1;
    const uint32_t sb0 = (uint32_t)(d0 - sa0), sb1 = (uint32_t)(d1 - sa1);
    GfTabMergeWindow w;
    w.a0 = sa0 - (sa0 > 0u), w.b0 = sb0 - (sb0 > 0u);
    w.a1 = sa1 < nA ? sa1 + 1u : nA, w.b1 = sb1 < nB ? sb1 + 1u : nB;
    w.pre = (sa0 > 0u) + (sb0 > 0u);
    return w;
}

// THE RUN: `steps` entries of the merged sequence from the cursor (ia, ib) on, by the pair rule; emit(k, symbol, count) for the
// run's k-th head.  Returns the heads.  The tables may be windows (gf_tab_merge_window) with the cursor counted inside them.
template <class Emit>
GF_HD uint32_t gf_tab_merge_run(const uint32_t *symA, const int32_t *cntA, uint32_t nA, const uint32_t *symB, const int32_t *cntB, uint32_t nB,
                                uint32_t ia, uint32_t ib, uint32_t steps, Emit emit)
{
    // the entry in front of the cursor: the later one of A's last and B's last, which is the one with the larger symbol (B's of equals)
    bool hasPrev = ia > 0u || ib > 0u;
    uint32_t prev = ia > 0u ? symA[ia - 1u] : 0u;
    if (ib > 0u && (ia == 0u || symB[ib - 1u] >= prev)) prev = symB[ib - 1u];
    uint32_t heads = 0;
    for (uint32_t k = 0; k < steps && (ia < nA || ib < nB); k++) {
        const bool isA = gf_tab_merge_next_is_a(symA, nA, symB, nB, ia, ib);
        const uint32_t sym = isA ? symA[ia] : symB[ib];
        int32_t cnt = isA ? cntA[ia] : cntB[ib];
        ia += isA, ib += !isA;
        if (!hasPrev || sym != prev) {
            if (ia < nA || ib < nB) {                                      // one entry ahead
                const bool nextA = gf_tab_merge_next_is_a(symA, nA, symB, nB, ia, ib);
                if ((nextA ? symA[ia] : symB[ib]) == sym) cnt = (int32_t)((uint32_t)cnt + (uint32_t)(nextA ? cntA[ia] : cntB[ib]));
            }
            emit(heads, sym, cnt);
            heads++;
        }
        hasPrev = true, prev = sym;
    }
    return heads;
}

// the scalars of a table are taken over its entries with count > 0 alone, as the reference's walk over its count file does
// (EntropyTabulator.java:278-292): a count that wrapped to <= 0 keeps its entry and counts in n_symbols only
GF_HD void gf_tab_count_scalars(int32_t count, uint32_t &unique, uint32_t &repeated, int32_t &most)
{
    if (count <= 0) return;
    unique += count == 1, repeated += count != 1;
    most = count > most ? count : most;
}

// the summary of a merge, but for the scalars taken over the entries: n_samples is the int64 sum, bit 0 of reserved
// (GF_TAB_SYM_INPUT_TRUNCATED) says that an input did not hold all of its symbols (or said so itself)
GF_HD void gf_tab_merge_summary(GfTabSymbols &out, const GfTabSymbols *a, uint32_t nA, const GfTabSymbols *b, uint32_t nB, uint64_t nHeads, uint64_t cap)
{
    int32_t flag = 0;
    int64_t samples = 0;
    if (a) samples = (int64_t)((uint64_t)samples + (uint64_t)a->nSamples), flag |= (a->reserved & 1) | ((int64_t)nA < a->nSymbols);
    if (b) samples = (int64_t)((uint64_t)samples + (uint64_t)b->nSamples), flag |= (b->reserved & 1) | ((int64_t)nB < b->nSymbols);
    out.nSamples = samples, out.nSymbols = (int64_t)nHeads, out.nUnique = 0, out.nRepeated = 0;
    out.nWritten = (int64_t)(nHeads < cap ? nHeads : cap), out.maxCount = 0, out.reserved = flag;
}

// a SHORT cell's counter among the 65,536: its bits as a uint16, which is the ascending unsigned order of the sign-extended symbols
// (0 .. 32,767 in front of 0xFFFF8000 .. 0xFFFFFFFF); and its counter in the workgroup's window, or >= the window's size
#define GF_TAB_SHORT_WIN (GF_TAB_SHORT_WIN_HI - GF_TAB_SHORT_WIN_LO + 1)
GF_HD uint32_t gf_tab_short_slot(int16_t v) { return (uint32_t)(uint16_t)v; }
GF_HD uint32_t gf_tab_short_win_slot(int16_t v) { return (uint32_t)((int32_t)v - (GF_TAB_SHORT_WIN_LO)); }
GF_HD int16_t gf_tab_short_of_win_slot(uint32_t w) { return (int16_t)((int32_t)w + (GF_TAB_SHORT_WIN_LO)); }
