// CPU harness for gridfour_amd/csrc/gvrs_tabulate_common.h, the host/device-shared restatement of the reference's data assessment
// (InputDataStatCollector.java:55-85, PackageData.java:504-533, EntropyTabulator.java:229-236): the same functions the kernels
// inline, compiled with g++ and called cell by cell.  Built as a small shared library by tests/tabulate_cases.py (g++ -O2
// -ffp-contract=off) for tests/test_tabulate_shared_header.py and for tools/tabulate_rate.py (the host loop a caller has without
// the kernels: th_dense on several threads).
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../gridfour_amd/csrc/gvrs_tabulate_common.h"

namespace {

// cells [i0, i1) in order: their part, their counters added to counter
template <typename T>
void cells(const GfTabDenseGeom &g, const T *block, int64_t i0, int64_t i1, int32_t *counter, GfTabPart<double> &out)
{
    GfTabPart<T> p;
    gf_tab_part_start(p);
    for (int64_t i = i0; i < i1; i++) {
        const int32_t index = gf_tab_cell(g, block[i], g.firstCell + i, p);
        if (index >= 0) counter[index] = (int32_t)((uint32_t)counter[index] + 1u);
    }
    out = gf_tab_widen(p);
}

void part(const GfTabDenseGeom &g, const void *block, int64_t i0, int64_t i1, int32_t *counter, GfTabPart<double> &out)
{
    if (g.elemType == 0) cells(g, (const int32_t *)block, i0, i1, counter, out);
    else if (g.elemType == 1) cells(g, (const int16_t *)block, i0, i1, counter, out);
    else cells(g, (const float *)block, i0, i1, counter, out);
}

}  // namespace

extern "C" {

int32_t th_java_int(double x) { return gf_tab_java_int(x); }

void th_plan(int32_t defMin, int32_t defMax, double scale, int32_t *nCounter, int32_t *base, double *scaleUsed)
{
    const GfTabPlan p = gf_tab_plan(defMin, defMax, scale);
    *nCounter = p.nCounter, *base = p.base, *scaleUsed = p.scaleUsed;
}

// the sample of a value, and of an int cell at scale 1 by the form without FP64: the two must agree on every int
int32_t th_sample(double v, double scaleUsed) { return gf_tab_sample(v, scaleUsed); }
int32_t th_sample_unit(int32_t v) { return gf_tab_sample_unit(v); }
int32_t th_index(int32_t sample, int32_t base, int32_t nCounter) { return gf_tab_index(sample, base, nCounter); }

uint32_t th_symbol_i16(int16_t v) { return gf_tab_symbol_i16(v); }
uint32_t th_symbol_i32(int32_t v) { return gf_tab_symbol_i32(v); }

// one call of the dense form: counter[0 .. g.nCounter] added to (zeroed first unless accumulating), *summary written (merged with
// what it held when accumulating).  nThreads < 2: the calling thread alone; else the cells in nThreads runs with counters of
// their own, merged in order
void th_dense(const GfTabDenseGeom *g, const void *block, int32_t *counter, GfTabSummary *summary, int accumulate, int nThreads)
{
    const size_t nBins = (size_t)g->nCounter + 1;
    if (!accumulate)
        for (size_t i = 0; i < nBins; i++) counter[i] = 0;
    GfTabPart<double> all;
    gf_tab_part_start(all);
    if (nThreads < 2) {
        part(*g, block, 0, g->nCells, counter, all);
    } else {
        std::vector<std::vector<int32_t>> own(nThreads, std::vector<int32_t>(nBins, 0));
        std::vector<GfTabPart<double>> parts(nThreads);
        std::vector<std::thread> th;
        for (int w = 0; w < nThreads; w++) {
            const int64_t i0 = g->nCells * w / nThreads, i1 = g->nCells * (w + 1) / nThreads;
            th.emplace_back([=, &own, &parts]() { part(*g, block, i0, i1, own[w].data(), parts[w]); });
        }
        for (auto &x : th) x.join();
        for (int w = 0; w < nThreads; w++) {
            gf_tab_part_merge(all, parts[w]);
            for (size_t i = 0; i < nBins; i++) counter[i] = (int32_t)((uint32_t)counter[i] + (uint32_t)own[w][i]);
        }
    }
    gf_tab_finish(*summary, all, accumulate, g->nCells);
}

size_t th_geom_bytes(void) { return sizeof(GfTabDenseGeom); }
size_t th_summary_bytes(void) { return sizeof(GfTabSummary); }

}  // extern "C"
