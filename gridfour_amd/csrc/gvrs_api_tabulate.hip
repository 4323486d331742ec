// gvrs_api_tabulate.hip -- what is in a grid block: the reference's data assessment over blocks that lie in device memory
// (gf_block_tabulate_dense_dev, gf_block_tabulate_symbols_dev) or in host memory (the forms without _dev, staged through the
// context), the plan arithmetic (gf_tab_dense_plan_of) and the two entropy sums over a table of counts (gf_tab_entropy_counts).
// The device forms check their arguments, fill in the kernels' arguments and launch (gvrs_tabulate.hip): they never synchronise.
// Reference: demo/src/main/java/org/gridfour/demo/globalDEM/InputDataStatCollector.java:55-108, PackageData.java:445-448, :504-533,
// demo/src/main/java/org/gridfour/demo/entropy/EntropyTabulator.java:227-297, core/.../util/KahanSummation.java:63-69.

#include "gvrs_api_internal.h"

static_assert(sizeof(gf_tab_summary) == sizeof(GfTabSummary) && sizeof(gf_tab_symbols) == sizeof(GfTabSymbols), "the kernels write the ABI's structs");
#define TAB_SAME_FIELD(abi, f, mine, g) static_assert(offsetof(abi, f) == offsetof(mine, g) && sizeof(abi::f) == sizeof(mine::g), #abi "::" #f)
TAB_SAME_FIELD(gf_tab_summary, n_cells, GfTabSummary, nCells);
TAB_SAME_FIELD(gf_tab_summary, n_skipped, GfTabSummary, nSkipped);
TAB_SAME_FIELD(gf_tab_summary, n_samples, GfTabSummary, nSamples);
TAB_SAME_FIELD(gf_tab_summary, sum_samples, GfTabSummary, sumSamples);
TAB_SAME_FIELD(gf_tab_summary, sum_i, GfTabSummary, sumI);
TAB_SAME_FIELD(gf_tab_summary, min, GfTabSummary, mn);
TAB_SAME_FIELD(gf_tab_summary, max, GfTabSummary, mx);
TAB_SAME_FIELD(gf_tab_summary, min_at, GfTabSummary, mnAt);
TAB_SAME_FIELD(gf_tab_summary, max_at, GfTabSummary, mxAt);
TAB_SAME_FIELD(gf_tab_symbols, n_samples, GfTabSymbols, nSamples);
TAB_SAME_FIELD(gf_tab_symbols, n_symbols, GfTabSymbols, nSymbols);
TAB_SAME_FIELD(gf_tab_symbols, n_unique, GfTabSymbols, nUnique);
TAB_SAME_FIELD(gf_tab_symbols, n_repeated, GfTabSymbols, nRepeated);
TAB_SAME_FIELD(gf_tab_symbols, n_written, GfTabSymbols, nWritten);
TAB_SAME_FIELD(gf_tab_symbols, max_count, GfTabSymbols, maxCount);
TAB_SAME_FIELD(gf_tab_symbols, reserved, GfTabSymbols, reserved);
#undef TAB_SAME_FIELD

namespace {

constexpr int TAB_FLAGS = GF_TAB_ACCUMULATE | GF_TAB_SKIP_FILL;

// spec alone: ARG, UNSUPPORTED or the plan
gf_status tabPlan(const gf_tab_dense *spec, gf_tab_dense_plan &plan)
{
    if (!spec || !(spec->scale > 0.0)) return GF_ERR_ARG;                       // (a NaN scale fails the comparison)
    const GfTabPlan p = gf_tab_plan(spec->def_min, spec->def_max, spec->scale);
    if (p.nCounter < 0) return GF_ERR_ARG;
    plan.n_counter = p.nCounter, plan.base = p.base, plan.n_bins = (int64_t)p.nCounter + 1, plan.scale_used = p.scaleUsed;
    return plan.n_bins > GF_TAB_MAX_BINS ? GF_ERR_UNSUPPORTED : GF_OK;
}

// what the host can check of a cell array
gf_status tabBlockArgs(const gf_context *c, int elemType, const void *block, int64_t nCells, const void *summary)
{
    if (!c || !block || !summary || elemType < GF_ELEM_INT || elemType > GF_ELEM_ICF || nCells < 0) return GF_ERR_ARG;
    if (((uintptr_t)block & 3) != 0 || ((uintptr_t)summary & 7) != 0) return GF_ERR_ARG;
    return GF_OK;
}

gf_status denseArgs(const gf_context *c, int elemType, int32_t fillI, int flags, const void *block, int64_t nCells, int64_t firstCell,
                    const gf_tab_dense *spec, const int32_t *counter, const gf_tab_summary *summary, gf_tab_dense_plan &plan)
{
    gf_status s = tabBlockArgs(c, elemType, block, nCells, summary);
    if (s != GF_OK) return s;
    if (!counter || ((uintptr_t)counter & 3) != 0 || firstCell < 0 || (flags & ~TAB_FLAGS) != 0) return GF_ERR_ARG;
    if (elemType == GF_ELEM_SHORT && (fillI < -32768 || fillI > 32767)) return GF_ERR_ARG;
    s = tabPlan(spec, plan);
    if (s == GF_ERR_ARG) return s;
    return firstOf(elemType == GF_ELEM_ICF || nCells > GF_TAB_MAX_CELLS ? GF_ERR_UNSUPPORTED : GF_OK, s);
}

// (the caller holds the lock and has checked the arguments)
gf_status denseLaunch(gf_context *c, hipStream_t st, int elemType, int32_t fillI, int flags, const void *dBlock, int64_t nCells, int64_t firstCell,
                      const gf_tab_dense_plan &plan, int32_t *dCounter, gf_tab_summary *dSummary)
{
    gf_status s = c->dTabPartials.ensure((size_t)GF_TAB_MAX_GROUPS * sizeof(GfTabPartial));
    if (s != GF_OK) return s;
    const int accumulate = (flags & GF_TAB_ACCUMULATE) != 0;
    if (!accumulate) GF_HIP(hipMemsetAsync(dCounter, 0, (size_t)plan.n_bins * 4, st));
    GfTabDenseArgs a{};
    a.g.nCells = nCells, a.g.firstCell = firstCell, a.g.scaleUsed = plan.scale_used, a.g.base = plan.base, a.g.nCounter = plan.n_counter;
    a.g.elemType = elemType, a.g.fillI = fillI, a.g.skipFill = (flags & GF_TAB_SKIP_FILL) != 0 && elemType != GF_ELEM_FLOAT;
    a.block = dBlock, a.counter = dCounter, a.partials = (GfTabPartial *)c->dTabPartials.p, a.summary = (GfTabSummary *)dSummary;
    a.accumulate = accumulate;
    GF_HIP(gf_launch_tabulate_dense(a, st));
    return GF_OK;
}

gf_status symbolsArgs(const gf_context *c, int elemType, const void *block, int64_t nCells, const uint32_t *symbols, const int32_t *counts,
                      size_t cap, const gf_tab_symbols *summary)
{
    const gf_status s = tabBlockArgs(c, elemType, block, nCells, summary);
    if (s != GF_OK) return s;
    if (cap > 0 && (!symbols || !counts)) return GF_ERR_ARG;
    if (cap > 0 && ((((uintptr_t)symbols) | ((uintptr_t)counts)) & 3) != 0) return GF_ERR_ARG;
    if (elemType == GF_ELEM_ICF || nCells > 0x7fffffffLL) return GF_ERR_UNSUPPORTED;
    return GF_OK;
}

gf_status symbolsLaunch(gf_context *c, hipStream_t st, int elemType, const void *dBlock, int64_t nCells, uint32_t *dSymbols, int32_t *dCounts, size_t cap,
                        gf_tab_symbols *dSummary)
{
    if (nCells == 0) {
        GF_HIP(hipMemsetAsync(dSummary, 0, sizeof(gf_tab_symbols), st));
        return GF_OK;
    }
    const uint32_t n = (uint32_t)nCells;
    const GfTabSortPlan p = gf_tab_sort_plan(n);
    Carve k;
    const size_t atA = k.add(((size_t)n + 1) * 4), atB = k.add((size_t)n * 4), atHist = k.add(p.histWords * 4), atSums = k.add(p.sumWords * 4);
    const size_t atHeads = k.add(p.nRunBlocks * 4), atSym = k.add(4);
    const gf_status s = c->dTabSort.ensure(k);
    if (s != GF_OK) return s;
    GfTabSymbolsArgs a{};
    a.elemType = elemType, a.block = dBlock, a.n = n;
    a.keysA = c->dTabSort.at<uint32_t>(atA), a.keysB = c->dTabSort.at<uint32_t>(atB), a.hist = c->dTabSort.at<uint32_t>(atHist);
    a.sums = c->dTabSort.at<uint32_t>(atSums), a.heads = c->dTabSort.at<uint32_t>(atHeads), a.nSym = c->dTabSort.at<uint32_t>(atSym);
    a.symbols = dSymbols, a.counts = dCounts, a.cap = cap, a.summary = (GfTabSymbols *)dSummary;
    GF_HIP(gf_launch_tab_symbols(a, st));
    return GF_OK;
}

size_t tabItemBytes(int elemType) { return elemType == GF_ELEM_SHORT ? 2 : 4; }

}  // namespace

extern "C" {

gf_status gf_tab_dense_plan_of(const gf_tab_dense *spec, gf_tab_dense_plan *plan)
{
    if (!plan) return GF_ERR_ARG;
    gf_tab_dense_plan p{};
    const gf_status s = tabPlan(spec, p);
    if (s == GF_OK) *plan = p;
    return s;
}

gf_status gf_block_tabulate_dense_dev(gf_context *c, void *stream, int elemType, int32_t fillI, int flags, const void *dBlock, int64_t nCells,
                                      int64_t firstCell, const gf_tab_dense *spec, int32_t *dCounter, gf_tab_summary *dSummary)
{
    gf_tab_dense_plan plan{};
    const gf_status s = denseArgs(c, elemType, fillI, flags, dBlock, nCells, firstCell, spec, dCounter, dSummary, plan);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    return denseLaunch(c, streamOf(c, stream), elemType, fillI, flags, dBlock, nCells, firstCell, plan, dCounter, dSummary);
}

gf_status gf_block_tabulate_dense(gf_context *c, int elemType, int32_t fillI, int flags, const void *block, int64_t nCells, int64_t firstCell,
                                  const gf_tab_dense *spec, int32_t *counter, gf_tab_summary *summary)
{
    gf_tab_dense_plan plan{};
    gf_status s = denseArgs(c, elemType, fillI, flags, block, nCells, firstCell, spec, counter, summary, plan);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    // staging: block | counters | summary (what an accumulating call adds to goes in first)
    const unsigned both = (flags & GF_TAB_ACCUMULATE) ? STAGE_IN | STAGE_OUT : STAGE_OUT;
    HostStage sg(c);
    const int blockP = sg.in(block, (size_t)nCells * tabItemBytes(elemType));
    const int counterP = sg.add(counter, (size_t)plan.n_bins * 4, both), summaryP = sg.add(summary, sizeof(gf_tab_summary), both);
    if ((s = sg.begin()) != GF_OK) return s;
    s = denseLaunch(c, c->stream, elemType, fillI, flags, sg.ptr<void>(blockP), nCells, firstCell, plan, sg.ptr<int32_t>(counterP),
                    sg.ptr<gf_tab_summary>(summaryP));
    return s != GF_OK ? s : sg.end();
}

gf_status gf_block_tabulate_symbols_dev(gf_context *c, void *stream, int elemType, const void *dBlock, int64_t nCells, uint32_t *dSymbols,
                                        int32_t *dCounts, size_t tableCap, gf_tab_symbols *dSummary)
{
    const gf_status s = symbolsArgs(c, elemType, dBlock, nCells, dSymbols, dCounts, tableCap, dSummary);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    return symbolsLaunch(c, streamOf(c, stream), elemType, dBlock, nCells, dSymbols, dCounts, tableCap, dSummary);
}

gf_status gf_block_tabulate_symbols(gf_context *c, int elemType, const void *block, int64_t nCells, uint32_t *symbols, int32_t *counts,
                                    size_t tableCap, gf_tab_symbols *summary)
{
    gf_status s = symbolsArgs(c, elemType, block, nCells, symbols, counts, tableCap, summary);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    // staging: block | symbols | counts | summary (a table holds n_cells entries at most); the summary says how much of the table counts
    const size_t cap = std::min(tableCap, (size_t)nCells);
    gf_tab_symbols got{};
    HostStage sg(c);
    const int blockP = sg.in(block, (size_t)nCells * tabItemBytes(elemType));
    const int symbolsP = sg.held(symbols, cap * 4), countsP = sg.held(counts, cap * 4), summaryP = sg.out(&got, sizeof(got));
    if ((s = sg.begin()) != GF_OK) return s;
    s = symbolsLaunch(c, c->stream, elemType, sg.ptr<void>(blockP), nCells, sg.ptr<uint32_t>(symbolsP), sg.ptr<int32_t>(countsP), cap,
                      sg.ptr<gf_tab_symbols>(summaryP));
    if (s != GF_OK || (s = sg.flush()) != GF_OK) return s;
    got.n_written = std::min<int64_t>(got.n_symbols, (int64_t)tableCap);
    if (got.n_written > 0) {
        if ((s = sg.fetch(symbolsP, (size_t)got.n_written * 4)) != GF_OK || (s = sg.fetch(countsP, (size_t)got.n_written * 4)) != GF_OK) return s;
        if ((s = sg.end()) != GF_OK) return s;
    }
    *summary = got;
    return got.n_symbols > (int64_t)tableCap ? GF_ERR_CAPACITY : GF_OK;
}

gf_status gf_tab_entropy_counts(const int32_t *counts, size_t n, int64_t nSamples, int kahan, double *entropy)
{
    if (!entropy || (n > 0 && !counts) || nSamples < 0 || (kahan != 0 && kahan != 1)) return GF_ERR_ARG;
    const double d = (double)nSamples;
    if (kahan) {
        // EntropyTabulator.java:265-297 with KahanSummation.add as written
        double c = 0.0, s = 0.0;
        for (size_t i = 0; i < n; i++)
            if (counts[i] > 0) {
                const double p = (double)counts[i] / d;
                const double a = -p * log(p);
                const double y = a - c;
                const double t = s + y;
                c = (t - s) - y;
                s = t;
            }
        *entropy = s / log(2.0);
    } else {
        // InputDataStatCollector.getEntropy (:87-101)
        if (nSamples == 0) {
            *entropy = 0.0;
            return GF_OK;
        }
        double sum = 0.0;
        for (size_t i = 0; i < n; i++)
            if (counts[i] > 0) {
                const double p = (double)counts[i] / d;
                sum += p * log(p);
            }
        *entropy = -sum / log(2.0);
    }
    return GF_OK;
}

}  // extern "C"
