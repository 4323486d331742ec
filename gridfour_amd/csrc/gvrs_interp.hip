// gvrs_interp.hip -- B-spline interpolation over a grid block in device memory: value, first and second derivatives and the unit
// normal at a batch of query points, bit for bit what the reference's GvrsInterpolatorBSpline computes point by point
// (gvrs/GvrsInterpolatorBSpline.java:283-334, :374-484; interpolation/InterpolatorBSpline.java:159-379).  The arithmetic is
// gvrs_interp_common.h, shared with the CPU harness; this file is the data path.
//
// k_interp_points, a lane per point.  Coordinates come in as coalesced 8-byte loads (points form) or are one product and one sum of
// the lane's lattice indices (a lattice with a column spacing per row; one with a single spacing goes to k_interp_lattice below).
// The sixteen samples are four 16-byte loads at 4-byte aligned addresses for INT, FLOAT and ICF cells, sixteen loads for SHORT
// cells and for a window that wraps; INT and SHORT cells are widened, and the fill turned into NaN, on their way into registers.
// Outputs are structure-of-arrays: a wave's stores to one array are 512 consecutive bytes (the normal, three doubles per point, is
// three stores 24 bytes apart).  A point that has no result, and an output the target does not compute, gets NaN: every item is
// written exactly once.  No LDS.

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_interp_common.h"

namespace {

constexpr uint32_t IP_THREADS = 256;

template <bool LATTICE>
__global__ __launch_bounds__(IP_THREADS) void k_interp_points(const GfInterpArgs a, const size_t first, const size_t end)
{
    const size_t t0 = first + ((size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x) * IP_THREADS;     // (workgroup-uniform)
    const size_t t = t0 + threadIdx.x;
    if (t >= end) return;
    double row, col, cs = a.g.colSpacing;
    if (LATTICE) {
        // (i, j) of point t: one 64-bit division for the workgroup; the lane is at most one row further when a row has 256 points
        // or more, and j0 + lane fits 32 bits otherwise
        const size_t i0 = t0 / a.latCols, jj = t0 - i0 * a.latCols + threadIdx.x;
        const size_t q = a.latCols >= IP_THREADS ? (size_t)(jj >= a.latCols) : (size_t)((uint32_t)jj / (uint32_t)a.latCols);
        const size_t i = i0 + q, j = jj - q * a.latCols;
        row = a.latRow0 + (double)i * a.latRowStep;
        col = a.latCol0 + (double)j * a.latColStep;
        if (a.colSpacing) cs = a.colSpacing[i];
    } else {
        row = a.rows[t];
        col = a.cols[t];
        if (a.colSpacing) cs = a.colSpacing[t];
    }
    GfInterpResult r;
    const int status = gf_interp_point(a.g, a.block, row, col, cs, a.normal != nullptr, r);
    a.z[t] = r.z;
    if (a.zx) a.zx[t] = r.zx;
    if (a.zy) a.zy[t] = r.zy;
    if (a.zxx) a.zxx[t] = r.zxx;
    if (a.zxy) a.zxy[t] = r.zxy;
    if (a.zyy) a.zyy[t] = r.zyy;
    if (a.normal) {
        double *__restrict__ o = a.normal + 3 * t;
        o[0] = r.normal[0], o[1] = r.normal[1], o[2] = r.normal[2];
    }
    if (a.status) a.status[t] = status;
}

// ------------------------------------------------------------------------------------------------
// k_interp_lattice: a workgroup per patch of IPL_ROWS x IPL_COLS lattice points, for a lattice with ONE column spacing.  What
// depends on the output column alone -- its coordinate, the window's columns and wrap split, u, b0..b3, bu*, buu*, the column's
// verdict -- is computed once per patch by the lanes of wave 0, one column each; what depends on the output row alone -- the
// coordinate, the window's rows, v, the p* family, the row's verdict -- by the first lanes of wave 1, one row each; both through
// the functions k_interp_points calls, so the two kernels cannot differ in a bit.  They lie in LDS (64 x 112 + 16 x 112 bytes).
// After the barrier lane l of wave w takes column l of the patch and rows w, w + 4, ...: its column's record once into
// registers, the row's record as an LDS broadcast, the sixteen samples, the sums.  Stores run along the rows of the output.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t IPL_ROWS = 16, IPL_COLS = 64;

struct IplAxis {                       // 112 bytes
    GfInterpBasis B;
    int32_t at, n1, status, pad;       // row0 / col0 of the window, the columns before the wrap, GF_IP_*
};

__global__ __launch_bounds__(IP_THREADS) void k_interp_lattice(const GfInterpArgs a, const size_t patchCols)
{
    __shared__ IplAxis sCol[IPL_COLS], sRow[IPL_ROWS];
    const size_t w = (size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x;
    const size_t pr = w / patchCols, pc = w - pr * patchCols;
    const size_t i0 = pr * IPL_ROWS, j0 = pc * IPL_COLS;
    if (i0 >= a.latRows) return;                                               // (the grid's padding; workgroup-uniform)
    const uint32_t tid = threadIdx.x;
    if (tid < IPL_COLS) {
        IplAxis x;
        double u = 0;
        x.at = 0, x.n1 = 4, x.pad = 0;
        x.status = gf_interp_window_col(a.g, a.latCol0 + (double)(j0 + tid) * a.latColStep, x.at, x.n1, u);
        if (x.status == GF_IP_OK) gf_interp_basis(u, a.g.colSpacing, a.g.target, x.B);
        sCol[tid] = x;
    } else if (tid < IPL_COLS + IPL_ROWS) {
        IplAxis x;
        double v = 0;
        x.at = 0, x.n1 = 4, x.pad = 0;
        x.status = gf_interp_window_row(a.g, a.latRow0 + (double)(i0 + (tid - IPL_COLS)) * a.latRowStep, x.at, v);
        if (x.status == GF_IP_OK) gf_interp_basis(v, a.g.rowSpacing, a.g.target, x.B);
        sRow[tid - IPL_COLS] = x;
    }
    __syncthreads();
    const size_t j = j0 + (tid & (IPL_COLS - 1));
    if (j >= a.latCols) return;
    const IplAxis c = sCol[tid & (IPL_COLS - 1)];
#pragma unroll 1
    for (uint32_t r = tid / IPL_COLS; r < IPL_ROWS && i0 + r < a.latRows; r += IP_THREADS / IPL_COLS) {
        const size_t t = (i0 + r) * a.latCols + j;
        GfInterpResult res;
        gf_interp_nullify(res);
        int status = gf_interp_window_status(sRow[r].status, c.status);
        if (status == GF_IP_OK && !gf_interp_window_in_block(a.g, sRow[r].at, c.at, c.n1)) status = GF_IP_ERR_BOUNDS;
        if (status == GF_IP_OK) {
            double z[16];
            gf_interp_samples(a.g, a.block, sRow[r].at, c.at, c.n1, z);
            gf_interp_sums(z, c.B, sRow[r].B, a.g.target, res);
            if (a.normal) gf_interp_unit_normal(res.zx, res.zy, res.normal);
        }
        a.z[t] = res.z;
        if (a.zx) a.zx[t] = res.zx;
        if (a.zy) a.zy[t] = res.zy;
        if (a.zxx) a.zxx[t] = res.zxx;
        if (a.zxy) a.zxy[t] = res.zxy;
        if (a.zyy) a.zyy[t] = res.zyy;
        if (a.normal) {
            double *__restrict__ o = a.normal + 3 * t;
            o[0] = res.normal[0], o[1] = res.normal[1], o[2] = res.normal[2];
        }
        if (a.status) a.status[t] = status;
    }
}

}  // namespace

// one launch per 2^20 x 65,535 workgroups (any point count fits a few launches; in practice one)
hipError_t gf_launch_interp(const GfInterpArgs &a, hipStream_t stream)
{
    if (!a.block || !a.z || (!a.rows && (a.latCols == 0 || a.latRows == 0))) return hipErrorInvalidValue;
    if (!a.rows && !a.colSpacing) {
        // the lattice kernel, when its patches fit one launch (a lattice beyond 2^46 points goes the other way)
        const size_t patchRows = (a.latRows + IPL_ROWS - 1) / IPL_ROWS, patchCols = (a.latCols + IPL_COLS - 1) / IPL_COLS;
        if (patchRows <= (((size_t)1 << 20) * 65535u) / patchCols) {
            hipLaunchKernelGGL(k_interp_lattice, gf_tile_grid(patchRows * patchCols), dim3(IP_THREADS), 0, stream, a, patchCols);
            return hipGetLastError();
        }
    }
    constexpr size_t perLaunch = ((size_t)1 << 20) * 65535u * IP_THREADS;
    for (size_t first = 0; first < a.nPoints; first += perLaunch) {
        const size_t n = a.nPoints - first < perLaunch ? a.nPoints - first : perLaunch;
        const dim3 grid = gf_tile_grid((n + IP_THREADS - 1) / IP_THREADS);
        if (a.rows) hipLaunchKernelGGL(k_interp_points<false>, grid, dim3(IP_THREADS), 0, stream, a, first, first + n);
        else hipLaunchKernelGGL(k_interp_points<true>, grid, dim3(IP_THREADS), 0, stream, a, first, first + n);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
