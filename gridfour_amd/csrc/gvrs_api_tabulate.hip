// gvrs_api_tabulate.hip -- what is in a grid block: the reference's data assessment over blocks that lie in device memory
// (gf_block_tabulate_dense_dev, gf_block_tabulate_symbols_dev) or in host memory (the forms without _dev, staged through the
// context), the plan arithmetic (gf_tab_dense_plan_of) and the two entropy sums over a table of counts (gf_tab_entropy_counts);
// two symbol tables merged (gf_tab_symbols_merge[_dev]), a strip's symbols counted onto a table (gf_block_tabulate_symbols_acc[_dev])
// and the same for a rectangle still in tile records (gf_block_read_tabulated_symbols_elems[_dev]).
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

// the parts of dTabSort that the sort and the runs of n cells take
struct TabSortParts {
    size_t atA, atB, atHist, atSums, atHeads, atSym;
};
TabSortParts tabSortParts(Carve &k, uint32_t n)
{
    const GfTabSortPlan p = gf_tab_sort_plan(n);
    TabSortParts t;
    t.atA = k.add(((size_t)n + 1) * 4), t.atB = k.add((size_t)n * 4), t.atHist = k.add(p.histWords * 4), t.atSums = k.add(p.sumWords * 4);
    t.atHeads = k.add(p.nRunBlocks * 4), t.atSym = k.add(4);
    return t;
}

// (dTabSort holds the parts; n >= 1)
gf_status sortLaunch(gf_context *c, hipStream_t st, const TabSortParts &t, int elemType, const void *dBlock, uint32_t n, uint32_t *dSymbols,
                     int32_t *dCounts, size_t cap, gf_tab_symbols *dSummary)
{
    GfTabSymbolsArgs a{};
    a.elemType = elemType, a.block = dBlock, a.n = n;
    a.keysA = c->dTabSort.at<uint32_t>(t.atA), a.keysB = c->dTabSort.at<uint32_t>(t.atB), a.hist = c->dTabSort.at<uint32_t>(t.atHist);
    a.sums = c->dTabSort.at<uint32_t>(t.atSums), a.heads = c->dTabSort.at<uint32_t>(t.atHeads), a.nSym = c->dTabSort.at<uint32_t>(t.atSym);
    a.symbols = dSymbols, a.counts = dCounts, a.cap = cap, a.summary = (GfTabSymbols *)dSummary;
    GF_HIP(gf_launch_tab_symbols(a, st));
    return GF_OK;
}

gf_status symbolsLaunch(gf_context *c, hipStream_t st, int elemType, const void *dBlock, int64_t nCells, uint32_t *dSymbols, int32_t *dCounts, size_t cap,
                        gf_tab_symbols *dSummary)
{
    if (nCells == 0) {
        GF_HIP(hipMemsetAsync(dSummary, 0, sizeof(gf_tab_symbols), st));
        return GF_OK;
    }
    Carve k;
    const TabSortParts t = tabSortParts(k, (uint32_t)nCells);
    const gf_status s = c->dTabSort.ensure(k);
    if (s != GF_OK) return s;
    return sortLaunch(c, st, t, elemType, dBlock, (uint32_t)nCells, dSymbols, dCounts, cap, dSummary);
}

// ---- tables merged, and a strip accumulated onto a table

constexpr size_t TAB_MAX_ENTRIES = 0x7fffffffu;        // of one input table: the merged sequence's positions are counted in 32 bits
constexpr size_t TAB_SHORT_SYMBOLS = 65536;
// the entries that the table of one strip can have
size_t tabStripCap(int elemType, int64_t nCells) { return elemType == GF_ELEM_SHORT ? std::min<size_t>((size_t)nCells, TAB_SHORT_SYMBOLS) : (size_t)nCells; }

struct TabTable {                                      // a table as a caller hands it over
    const uint32_t *sym;
    const int32_t *cnt;
    const gf_tab_symbols *sum;
    size_t cap;
};

bool tabOverlap(const void *p, size_t pBytes, const void *q, size_t qBytes)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && pBytes && qBytes && a < b + qBytes && b < a + pBytes;
}

// what the host can check of an output table against the input tables: ARG
gf_status tabOutArgs(const TabTable *in, int nIn, const uint32_t *symOut, const int32_t *cntOut, size_t capOut, const gf_tab_symbols *sumOut)
{
    if (!sumOut || ((uintptr_t)sumOut & 7) != 0 || (capOut > 0 && (!symOut || !cntOut))) return GF_ERR_ARG;
    if (capOut > 0 && ((((uintptr_t)symOut) | ((uintptr_t)cntOut)) & 3) != 0) return GF_ERR_ARG;
    for (int i = 0; i < nIn; i++) {
        if (in[i].cap > 0 && (!in[i].sym || !in[i].cnt)) return GF_ERR_ARG;
        if (in[i].cap > 0 && ((((uintptr_t)in[i].sym) | ((uintptr_t)in[i].cnt)) & 3) != 0) return GF_ERR_ARG;
        if (((uintptr_t)in[i].sum & 7) != 0) return GF_ERR_ARG;
    }
    // the outputs apart from one another and from every input
    const void *out[3] = {symOut, cntOut, sumOut};
    const size_t outBytes[3] = {capOut * 4, capOut * 4, sizeof(gf_tab_symbols)};
    if (tabOverlap(out[0], outBytes[0], out[1], outBytes[1]) || tabOverlap(out[0], outBytes[0], out[2], outBytes[2]) ||
        tabOverlap(out[1], outBytes[1], out[2], outBytes[2]))
        return GF_ERR_ARG;
    for (int i = 0; i < nIn; i++)
        for (int o = 0; o < 3; o++)
            if (tabOverlap(out[o], outBytes[o], in[i].sym, in[i].cap * 4) || tabOverlap(out[o], outBytes[o], in[i].cnt, in[i].cap * 4) ||
                tabOverlap(out[o], outBytes[o], in[i].sum, sizeof(gf_tab_symbols)))
                return GF_ERR_ARG;
    return GF_OK;
}

gf_status mergeArgs(const gf_context *c, const TabTable &a, const TabTable &b, const uint32_t *symOut, const int32_t *cntOut, size_t capOut,
                    const gf_tab_symbols *sumOut)
{
    if (!c || !a.sum || !b.sum) return GF_ERR_ARG;
    const TabTable in[2] = {a, b};
    const gf_status s = tabOutArgs(in, 2, symOut, cntOut, capOut, sumOut);
    if (s != GF_OK) return s;
    return a.cap > TAB_MAX_ENTRIES || b.cap > TAB_MAX_ENTRIES ? GF_ERR_UNSUPPORTED : GF_OK;
}

// the in-table of an accumulating call: NULL arrays, a NULL summary or cap_in == 0 say "empty"
gf_status accArgs(const gf_context *c, int elemType, const void *block, int64_t nCells, TabTable &in, const uint32_t *symOut, const int32_t *cntOut,
                  size_t capOut, const gf_tab_symbols *sumOut)
{
    if (!c || !block || elemType < GF_ELEM_INT || elemType > GF_ELEM_ICF || nCells < 0) return GF_ERR_ARG;
    if (((uintptr_t)block & (elemType == GF_ELEM_SHORT ? 1 : 3)) != 0) return GF_ERR_ARG;
    if (in.cap > 0 && (!in.sym) != (!in.cnt)) return GF_ERR_ARG;
    if (!in.sym || !in.sum) in.cap = 0;
    const gf_status s = tabOutArgs(&in, 1, symOut, cntOut, capOut, sumOut);
    if (s != GF_OK) return s;
    return elemType == GF_ELEM_ICF || nCells > 0x7fffffffLL || in.cap > TAB_MAX_ENTRIES ? GF_ERR_UNSUPPORTED : GF_OK;
}

struct TabMergeParts {
    size_t atSplits, atHeads, atSums, atSym;
};
TabMergeParts tabMergeParts(Carve &k, size_t capA, size_t capB)
{
    const size_t chunks = gf_tab_merge_chunks((uint32_t)capA, (uint32_t)capB);
    TabMergeParts t;
    t.atSplits = k.add((chunks + 1) * 4), t.atHeads = k.add(chunks * 4), t.atSums = k.add((chunks + GF_TAB_SCAN_BLOCK - 1) / GF_TAB_SCAN_BLOCK * 4), t.atSym = k.add(4);
    return t;
}

// (dTabSort holds the parts; a summary that is null: that table is empty)
gf_status mergeLaunch(gf_context *c, hipStream_t st, const TabMergeParts &t, const TabTable &a, const TabTable &b, unsigned noSamplesIsEmpty,
                      uint32_t *dSymOut, int32_t *dCntOut, size_t capOut, gf_tab_symbols *dSumOut)
{
    GfTabMergeArgs m{};
    m.symA = a.sym, m.cntA = a.cnt, m.sumA = (const GfTabSymbols *)a.sum, m.capA = (uint32_t)a.cap;
    m.symB = b.sym, m.cntB = b.cnt, m.sumB = (const GfTabSymbols *)b.sum, m.capB = (uint32_t)b.cap;
    m.noSamplesIsEmpty = noSamplesIsEmpty;
    m.splits = c->dTabSort.at<uint32_t>(t.atSplits), m.heads = c->dTabSort.at<uint32_t>(t.atHeads), m.sums = c->dTabSort.at<uint32_t>(t.atSums), m.nSym = c->dTabSort.at<uint32_t>(t.atSym);
    m.symbols = dSymOut, m.counts = dCntOut, m.cap = capOut, m.summary = (GfTabSymbols *)dSumOut;
    GF_HIP(gf_launch_tab_merge(m, st));
    return GF_OK;
}

gf_status mergeDev(gf_context *c, hipStream_t st, const TabTable &a, const TabTable &b, uint32_t *dSymOut, int32_t *dCntOut, size_t capOut,
                   gf_tab_symbols *dSumOut)
{
    Carve k;
    const TabMergeParts t = tabMergeParts(k, a.cap, b.cap);
    const gf_status s = c->dTabSort.ensure(k);
    return s != GF_OK ? s : mergeLaunch(c, st, t, a, b, 0u, dSymOut, dCntOut, capOut, dSumOut);
}

// The strip into a table of the context (INT / FLOAT: the sort and the runs; SHORT: the counters), then that table merged with the
// caller's: one layout of dTabSort for both steps.  (The caller holds the lock and has checked the arguments.)
gf_status accDev(gf_context *c, hipStream_t st, int elemType, const void *dBlock, int64_t nCells, const TabTable &in, uint32_t *dSymOut,
                 int32_t *dCntOut, size_t capOut, gf_tab_symbols *dSumOut)
{
    const uint32_t n = (uint32_t)nCells;
    const bool counters = elemType == GF_ELEM_SHORT;
    const size_t stripCap = tabStripCap(elemType, nCells);
    Carve k;
    TabSortParts sp{};
    size_t atCounter = 0;
    if (n && counters) atCounter = k.add(TAB_SHORT_SYMBOLS * 4);
    else if (n) sp = tabSortParts(k, n);
    const size_t atSym = k.add(stripCap * 4), atCnt = k.add(stripCap * 4), atSum = k.add(sizeof(gf_tab_symbols));
    const TabMergeParts mp = tabMergeParts(k, in.cap, stripCap);
    gf_status s = c->dTabSort.ensure(k);
    if (s != GF_OK) return s;
    TabTable strip{c->dTabSort.at<uint32_t>(atSym), c->dTabSort.at<int32_t>(atCnt), n ? c->dTabSort.at<gf_tab_symbols>(atSum) : nullptr, stripCap};
    if (n && counters) {
        GfTabShortArgs a{};
        a.block = dBlock, a.n = n, a.counter = c->dTabSort.at<int32_t>(atCounter);
        a.symbols = const_cast<uint32_t *>(strip.sym), a.counts = const_cast<int32_t *>(strip.cnt), a.cap = stripCap;
        a.summary = (GfTabSymbols *)const_cast<gf_tab_symbols *>(strip.sum);
        GF_HIP(gf_launch_tab_short(a, st));
    } else if (n) {
        s = sortLaunch(c, st, sp, elemType, dBlock, n, const_cast<uint32_t *>(strip.sym), const_cast<int32_t *>(strip.cnt), stripCap,
                       const_cast<gf_tab_symbols *>(strip.sum));
        if (s != GF_OK) return s;
    }
    return mergeLaunch(c, st, mp, in, strip, 1u, dSymOut, dCntOut, capOut, dSumOut);
}

// the entries of a table in host memory that count
size_t tabHostLen(const TabTable &t, bool noSamplesIsEmpty)
{
    if (!t.sum || (noSamplesIsEmpty && t.sum->n_samples == 0) || t.sum->n_written <= 0) return 0;
    return std::min<uint64_t>((uint64_t)t.sum->n_written, t.cap);
}

// What the host forms share.  staging: what declare() adds (a block; records) | A's symbols, counts, summary | B's | the out table's |
// its summary; an input goes up with the entries that count and as a table of exactly that many, the out table holds no more than
// the inputs and `most` more entries can give
template <class Declare, class Launch>
gf_status tabHostTables(gf_context *c, const TabTable *in, int nIn, bool noSamplesIsEmpty, size_t most, uint32_t *symOut, int32_t *cntOut,
                        size_t capOut, gf_tab_symbols *sumOut, Declare declare, Launch launch)
{
    GF_HIP(hipSetDevice(c->device));
    HostStage sg(c);
    declare(sg);
    int symP[2] = {0, 0}, cntP[2] = {0, 0}, sumP[2] = {0, 0};
    size_t len[2] = {0, 0};
    for (int i = 0; i < nIn; i++) {
        len[i] = tabHostLen(in[i], noSamplesIsEmpty);
        most += len[i];
        symP[i] = sg.in(in[i].sym, len[i] * 4), cntP[i] = sg.in(in[i].cnt, len[i] * 4);
        sumP[i] = sg.in(in[i].sum, in[i].sum ? sizeof(gf_tab_symbols) : 0);
    }
    const size_t cap = std::min(capOut, most);
    gf_tab_symbols got{};
    const int symOutP = sg.held(symOut, cap * 4), cntOutP = sg.held(cntOut, cap * 4), sumOutP = sg.out(&got, sizeof(got));
    gf_status s = sg.begin();
    if (s != GF_OK) return s;
    TabTable d[2] = {};
    for (int i = 0; i < nIn; i++)
        d[i] = TabTable{sg.ptr<uint32_t>(symP[i]), sg.ptr<int32_t>(cntP[i]), in[i].sum ? sg.ptr<gf_tab_symbols>(sumP[i]) : nullptr, len[i]};
    s = launch(sg, d, sg.ptr<uint32_t>(symOutP), sg.ptr<int32_t>(cntOutP), cap, sg.ptr<gf_tab_symbols>(sumOutP));
    if (s != GF_OK || (s = sg.flush()) != GF_OK) return s;
    got.n_written = std::min<int64_t>(got.n_symbols, (int64_t)capOut);
    if (got.n_written > 0) {
        if ((s = sg.fetch(symOutP, (size_t)got.n_written * 4)) != GF_OK || (s = sg.fetch(cntOutP, (size_t)got.n_written * 4)) != GF_OK) return s;
        if ((s = sg.end()) != GF_OK) return s;
    }
    *sumOut = got;
    return got.n_symbols > (int64_t)capOut || (got.reserved & GF_TAB_SYM_INPUT_TRUNCATED) ? GF_ERR_CAPACITY : GF_OK;
}

size_t tabItemBytes(int elemType) { return elemType == GF_ELEM_SHORT ? 2 : 4; }

// the composed read's argument checks: the block read's on the elements as given, then the accumulate form's on element `which`
// with an ICF element taken as its INT codes (asCodes, fill: as dsReadArgs of gvrs_api_downsample.hip gives them)
gf_status readTabArgs(const gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems, const gf_grid_spec *grid,
                      const gf_rect *rect, size_t nRecords, const uint8_t *blob, bool blobOnDevice, const uint64_t *offsets, int which, TabTable &in,
                      const uint32_t *symOut, const int32_t *cntOut, size_t capOut, const gf_tab_symbols *sumOut, const int32_t *status, GfBlockGeom &g,
                      gf_elem_spec *asCodes, uint32_t *fill)
{
    void *standIn[GF_MAX_ELEMS];                       // (the block read checks its output pointers: the blocks are the context's here)
    for (int e = 0; e < GF_MAX_ELEMS; e++) standIn[e] = &g;
    gf_status s = blockReadArgs(c, codecs, nCodecs, elems, nElems, grid, rect, nRecords, blob, blobOnDevice, offsets, standIn, status, g, fill);
    if (s == GF_ERR_ARG) return s;
    if (which < 0 || which >= nElems) return GF_ERR_ARG;
    for (int e = 0; e < nElems; e++) {
        asCodes[e] = elems[e];
        if (elems[e].type == GF_ELEM_ICF) asCodes[e].type = GF_ELEM_INT;
    }
    s = firstOf(s, accArgs(c, asCodes[which].type, &g, (int64_t)rect->n_rows * (int64_t)rect->n_cols, in, symOut, cntOut, capOut, sumOut));
    return s != GF_OK ? s : elemFills(asCodes, nElems, fill);
}

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

gf_status gf_tab_symbols_merge_dev(gf_context *c, const uint32_t *dSymA, const int32_t *dCntA, const gf_tab_symbols *dSumA, size_t capA,
                                   const uint32_t *dSymB, const int32_t *dCntB, const gf_tab_symbols *dSumB, size_t capB, uint32_t *dSymOut,
                                   int32_t *dCntOut, size_t tableCap, gf_tab_symbols *dSumOut)
{
    const TabTable a{dSymA, dCntA, dSumA, capA}, b{dSymB, dCntB, dSumB, capB};
    const gf_status s = mergeArgs(c, a, b, dSymOut, dCntOut, tableCap, dSumOut);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    return mergeDev(c, c->stream, a, b, dSymOut, dCntOut, tableCap, dSumOut);
}

gf_status gf_tab_symbols_merge(gf_context *c, const uint32_t *symA, const int32_t *cntA, const gf_tab_symbols *sumA, size_t capA, const uint32_t *symB,
                               const int32_t *cntB, const gf_tab_symbols *sumB, size_t capB, uint32_t *symOut, int32_t *cntOut, size_t tableCap,
                               gf_tab_symbols *sumOut)
{
    const TabTable in[2] = {{symA, cntA, sumA, capA}, {symB, cntB, sumB, capB}};
    const gf_status s = mergeArgs(c, in[0], in[1], symOut, cntOut, tableCap, sumOut);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    return tabHostTables(c, in, 2, false, 0, symOut, cntOut, tableCap, sumOut, [](HostStage &) {},
                         [&](HostStage &, const TabTable *d, uint32_t *dSym, int32_t *dCnt, size_t cap, gf_tab_symbols *dSum) {
                             return mergeDev(c, c->stream, d[0], d[1], dSym, dCnt, cap, dSum);
                         });
}

gf_status gf_block_tabulate_symbols_acc_dev(gf_context *c, int elemType, const void *dBlock, int64_t nCells, const uint32_t *dSymIn,
                                            const int32_t *dCntIn, const gf_tab_symbols *dSumIn, size_t capIn, uint32_t *dSymOut, int32_t *dCntOut,
                                            size_t capOut, gf_tab_symbols *dSumOut)
{
    TabTable in{dSymIn, dCntIn, dSumIn, capIn};
    const gf_status s = accArgs(c, elemType, dBlock, nCells, in, dSymOut, dCntOut, capOut, dSumOut);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    return accDev(c, c->stream, elemType, dBlock, nCells, in, dSymOut, dCntOut, capOut, dSumOut);
}

gf_status gf_block_tabulate_symbols_acc(gf_context *c, int elemType, const void *block, int64_t nCells, const uint32_t *symIn, const int32_t *cntIn,
                                        const gf_tab_symbols *sumIn, size_t capIn, uint32_t *symOut, int32_t *cntOut, size_t capOut,
                                        gf_tab_symbols *sumOut)
{
    TabTable in{symIn, cntIn, sumIn, capIn};
    const gf_status s = accArgs(c, elemType, block, nCells, in, symOut, cntOut, capOut, sumOut);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    int blockP = 0;
    return tabHostTables(c, &in, 1, true, tabStripCap(elemType, nCells), symOut, cntOut, capOut, sumOut,
                         [&](HostStage &sg) { blockP = sg.in(block, (size_t)nCells * tabItemBytes(elemType)); },
                         [&](HostStage &sg, const TabTable *d, uint32_t *dSym, int32_t *dCnt, size_t cap, gf_tab_symbols *dSum) {
                             return accDev(c, c->stream, elemType, sg.ptr<void>(blockP), nCells, d[0], dSym, dCnt, cap, dSum);
                         });
}

gf_status gf_block_read_tabulated_symbols_elems_dev(gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems,
                                                    const gf_grid_spec *grid, const gf_rect *rect, size_t nRecords, const uint8_t *dBlob,
                                                    size_t blobBytes, const uint64_t *dOffsets, int verifyChecksum, int which,
                                                    const uint32_t *dSymIn, const int32_t *dCntIn, const gf_tab_symbols *dSumIn, size_t capIn,
                                                    uint32_t *dSymOut, int32_t *dCntOut, size_t capOut, gf_tab_symbols *dSumOut, int32_t *dStatus)
{
    GfBlockGeom g{};
    uint32_t fill[GF_MAX_ELEMS];
    gf_elem_spec asCodes[GF_MAX_ELEMS];
    TabTable in{dSymIn, dCntIn, dSumIn, capIn};
    gf_status s = readTabArgs(c, codecs, nCodecs, elems, nElems, grid, rect, nRecords, dBlob, true, dOffsets, which, in, dSymOut, dCntOut, capOut,
                              dSumOut, dStatus, g, asCodes, fill);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    GF_HIP(hipSetDevice(c->device));
    const size_t nCells = (size_t)rect->n_rows * (size_t)rect->n_cols;
    void *dFull[GF_MAX_ELEMS];
    if ((s = elemArrays(c->dTabBlocks, asCodes, nElems, nCells, dFull)) != GF_OK) return s;
    s = blockReadDev(c, nullptr, codecs, nCodecs, asCodes, nElems, g, fill, nRecords, dBlob, blobBytes, dOffsets, verifyChecksum, dFull, dStatus);
    if (s != GF_OK) return s;
    return accDev(c, c->stream, asCodes[which].type, dFull[which], (int64_t)nCells, in, dSymOut, dCntOut, capOut, dSumOut);
}

gf_status gf_block_read_tabulated_symbols_elems(gf_context *c, const int *codecs, int nCodecs, const gf_elem_spec *elems, int nElems,
                                                const gf_grid_spec *grid, const gf_rect *rect, size_t nRecords, const uint8_t *blob,
                                                const uint64_t *offsets, int verifyChecksum, int which, const uint32_t *symIn, const int32_t *cntIn,
                                                const gf_tab_symbols *sumIn, size_t capIn, uint32_t *symOut, int32_t *cntOut, size_t capOut,
                                                gf_tab_symbols *sumOut, int32_t *status)
{
    GfBlockGeom g{};
    uint32_t fill[GF_MAX_ELEMS];
    gf_elem_spec asCodes[GF_MAX_ELEMS];
    TabTable in{symIn, cntIn, sumIn, capIn};
    gf_status s = readTabArgs(c, codecs, nCodecs, elems, nElems, grid, rect, nRecords, blob, false, offsets, which, in, symOut, cntOut, capOut, sumOut,
                              status, g, asCodes, fill);
    if (s != GF_OK) return s;
    GF_CTX_LOCK(c);
    const size_t blobBytes = nRecords ? (size_t)offsets[nRecords] : 0;
    const size_t nCells = (size_t)rect->n_rows * (size_t)rect->n_cols;
    int blobP = 0, offsetsP = 0, statusP = 0;
    return tabHostTables(c, &in, 1, true, tabStripCap(asCodes[which].type, (int64_t)nCells), symOut, cntOut, capOut, sumOut,
                         [&](HostStage &sg) {
                             blobP = sg.in(blob, blobBytes, 32), offsetsP = sg.in(offsets, nRecords ? (nRecords + 1) * 8 : 0);
                             statusP = sg.out(status, (size_t)nElems * nRecords * 4);
                         },
                         [&](HostStage &sg, const TabTable *d, uint32_t *dSym, int32_t *dCnt, size_t cap, gf_tab_symbols *dSum) {
                             void *dFull[GF_MAX_ELEMS];
                             gf_status r = elemArrays(c->dTabBlocks, asCodes, nElems, nCells, dFull);
                             if (r != GF_OK) return r;
                             r = blockReadDev(c, c->stream, codecs, nCodecs, asCodes, nElems, g, fill, nRecords, sg.ptr<uint8_t>(blobP), blobBytes,
                                              sg.ptr<uint64_t>(offsetsP), verifyChecksum, dFull, sg.ptr<int32_t>(statusP));
                             if (r != GF_OK) return r;
                             return accDev(c, c->stream, asCodes[which].type, dFull[which], (int64_t)nCells, d[0], dSym, dCnt, cap, dSum);
                         });
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
