// CPU harness for gridfour_amd/csrc/gvrs_interp_common.h, the host/device-shared restatement of the reference's B-spline
// interpolator: the same functions the kernels inline, compiled with g++ and called point by point.  Built as a small shared
// library by tests/test_interp_shared_header.py (g++ -O2 -ffp-contract=off) and by tools/interp_rate.py (the host route a caller
// has without the kernels: ih_interp_points on several threads).
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../gridfour_amd/csrc/gvrs_interp_common.h"

namespace {

struct Out {
    double *z, *zx, *zy, *zxx, *zxy, *zyy, *normal;
    int32_t *status;
};

void range(const GfInterpGeom &g, const void *block, size_t t0, size_t t1, const double *rows, const double *cols, const double *cs, const Out &o)
{
    for (size_t t = t0; t < t1; t++) {
        GfInterpResult r;
        const int st = gf_interp_point(g, block, rows[t], cols[t], cs ? cs[t] : g.colSpacing, o.normal != nullptr, r);
        o.z[t] = r.z;
        if (o.zx) o.zx[t] = r.zx;
        if (o.zy) o.zy[t] = r.zy;
        if (o.zxx) o.zxx[t] = r.zxx;
        if (o.zxy) o.zxy[t] = r.zxy;
        if (o.zyy) o.zyy[t] = r.zyy;
        if (o.normal) o.normal[3 * t] = r.normal[0], o.normal[3 * t + 1] = r.normal[1], o.normal[3 * t + 2] = r.normal[2];
        if (o.status) o.status[t] = st;
    }
}

}  // namespace

extern "C" {

// every point of a batch; outputs other than z may be null; nThreads < 2: the calling thread alone
void ih_interp_points(const GfInterpGeom *g, const void *block, size_t n, const double *rows, const double *cols, const double *colSpacing,
                      double *z, double *zx, double *zy, double *zxx, double *zxy, double *zyy, double *normal, int32_t *status, int nThreads)
{
    const Out o{z, zx, zy, zxx, zxy, zyy, normal, status};
    if (nThreads < 2) {
        range(*g, block, 0, n, rows, cols, colSpacing, o);
        return;
    }
    std::vector<std::thread> th;
    for (int w = 0; w < nThreads; w++) {
        const size_t t0 = n * (size_t)w / (size_t)nThreads, t1 = n * (size_t)(w + 1) / (size_t)nThreads;
        th.emplace_back([=, &o]() { range(*g, block, t0, t1, rows, cols, colSpacing, o); });
    }
    for (auto &x : th) x.join();
}

// the window alone: status, row0, col0, n1, u, v
int ih_window(const GfInterpGeom *g, double row, double col, int32_t *rc, double *uv)
{
    GfInterpWindow w{};
    const int st = gf_interp_window(*g, row, col, w);
    rc[0] = w.row0, rc[1] = w.col0, rc[2] = w.n1;
    uv[0] = w.u, uv[1] = w.v;
    return st;
}

size_t ih_geom_bytes(void) { return sizeof(GfInterpGeom); }

}  // extern "C"
