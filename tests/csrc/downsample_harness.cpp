// CPU harness for gridfour_amd/csrc/gvrs_downsample_common.h, the host/device-shared restatement of the reference's box average
// (ExampleDownsample.java:185-206): the same functions the kernels inline, compiled with g++ and called cell by cell.  Built as a
// small shared library by tests/downsample_cases.py (g++ -O2 -ffp-contract=off) for tests/test_downsample_shared_header.py and for
// tools/downsample_rate.py (the host route a caller has without the kernels: dh_downsample on several threads).
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../gridfour_amd/csrc/gvrs_downsample_common.h"

namespace {

void rows(const GfDsGeom &g, const void *block, void *out, int64_t i0, int64_t i1)
{
    for (int64_t i = i0; i < i1; i++)
        for (int64_t j = 0; j < g.outCols; j++) {
            const int64_t t = i * g.outCols + j;
            if (g.elemType == 0) ((int32_t *)out)[t] = gf_ds_cell_int32(g, (const int32_t *)block, i, j);
            else if (g.elemType == 1) ((int16_t *)out)[t] = gf_ds_cell_int16(g, (const int16_t *)block, i, j);
            else ((float *)out)[t] = gf_ds_cell_float(g, (const float *)block, i, j);
        }
}

}  // namespace

extern "C" {

// every output cell of a call; nThreads < 2: the calling thread alone
void dh_downsample(const GfDsGeom *g, const void *block, void *out, int nThreads)
{
    if (nThreads < 2) {
        rows(*g, block, out, 0, g->outRows);
        return;
    }
    std::vector<std::thread> th;
    for (int w = 0; w < nThreads; w++) {
        const int64_t i0 = g->outRows * w / nThreads, i1 = g->outRows * (w + 1) / nThreads;
        th.emplace_back([=]() { rows(*g, block, out, i0, i1); });
    }
    for (auto &x : th) x.join();
}

// the rectangle rule for one axis: out[0] = first coarse cell, out[1] = count
void dh_axis(int32_t at, int32_t n, int32_t f, int32_t *out) { gf_ds_axis(at, n, f, out[0], out[1]); }

size_t dh_geom_bytes(void) { return sizeof(GfDsGeom); }

}  // extern "C"
