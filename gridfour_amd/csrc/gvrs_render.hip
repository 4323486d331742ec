// gvrs_render.hip -- a grid block in device memory turned into ARGB words: the reference's colour palette lookup
// (imaging/palette/ColorPaletteTable.java:395-598) on the cells of a block, or on the B-spline surface over it with the shaded
// relief of the reference's demos (demo/.../globalDEM/ExtractData.java:394-419, demo/geoTiff/DemoCOG.java:405-441), bit for bit.
// The arithmetic is gvrs_render_common.h and gvrs_interp_common.h, shared with the CPU harnesses; this file is the data path.
//
// Every workgroup stages the palette -- keys[n] and recs[n], 80 bytes a record, dynamic LDS -- once; the binary search is at most
// 9 dependent LDS reads (n <= 256), the record another LDS read.  One int32 per pixel is stored: 4 bytes where the interpolator
// stores 24 to 48.

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_interp_common.h"
#include "gvrs_render_common.h"

namespace {

constexpr uint32_t RD_THREADS = 256;

extern __shared__ double sPal[];                   // keys[n] | recs[n]

__device__ __forceinline__ void stage_palette(const GfRenderPal &p)
{
    const uint32_t words = 10u * (uint32_t)p.head.n;
    for (uint32_t i = threadIdx.x; i < words; i += RD_THREADS) sPal[i] = p.table[i];
}
__device__ __forceinline__ uint32_t palette_argb(const GfRenderPal &p, double z, double shade, bool withShade)
{
    return gf_render_palette(p.head, sPal, reinterpret_cast<const GfPalRec *>(sPal + p.head.n), z, shade, withShade, p.unlimited != 0);
}

// ------------------------------------------------------------------------------------------------
// k_render_cells: cells -> argb.  The first `head` cells (0..3: up to where argb is 16-byte aligned) and the cells behind the last
// whole group of four are taken one by one by the first lanes of workgroup 0.  Between them lane by lane four consecutive cells:
// INT, FLOAT and ICF cells as one 16-byte load (the address is 4-byte aligned, which gfx950 serves), SHORT cells as one 8-byte load
// where the address is 8-byte aligned and four 2-byte loads otherwise (workgroup-uniform), doubles (GF_RENDER_ELEM_Z: z as the
// interpolator delivers it) as they are; four shades; one 16-byte store.  A workgroup takes RC_ITERS x 256 groups, so that the
// staged palette serves 4,096 cells.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t RC_ITERS = 4;

__device__ __forceinline__ double cell_z(const GfRenderCellsArgs &a, uint32_t bits)
{
    return a.elemType >= 2 ? gf_render_cell_f32(bits) : gf_render_cell_i32((int32_t)bits, a.fillI);
}
__device__ __forceinline__ double cell_at(const GfRenderCellsArgs &a, size_t i)
{
    if (a.elemType == GF_RENDER_ELEM_Z) return reinterpret_cast<const double *>(a.cells)[i];
    return cell_z(a, a.elemType == 1 ? (uint32_t)(int32_t) reinterpret_cast<const int16_t *>(a.cells)[i] : reinterpret_cast<const uint32_t *>(a.cells)[i]);
}

__global__ __launch_bounds__(RD_THREADS) void k_render_cells(const GfRenderCellsArgs a, const uint32_t head, const size_t nGroups)
{
    stage_palette(a.pal);
    __syncthreads();
    const size_t wg = (size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x;
    const uint32_t tid = threadIdx.x;
    const bool withShade = a.shade != nullptr;
    const size_t body = (size_t)head + 4 * nGroups;
    if (wg == 0 && tid < head + (uint32_t)(a.nCells - body)) {
        const size_t i = tid < head ? tid : body + (tid - head);
        a.argb[i] = palette_argb(a.pal, cell_at(a, i), withShade ? a.shade[i] : 0.0, withShade);
    }
    const bool shortAligned = ((uintptr_t)(reinterpret_cast<const int16_t *>(a.cells) + head) & 7u) == 0;
#pragma unroll 1
    for (uint32_t k = 0; k < RC_ITERS; k++) {
        const size_t g = (wg * RC_ITERS + k) * RD_THREADS + tid;
        if (g >= nGroups) return;
        const size_t at = (size_t)head + 4 * g;
        double z[4];
        if (a.elemType == GF_RENDER_ELEM_Z) {
#pragma unroll
            for (int j = 0; j < 4; j++) z[j] = reinterpret_cast<const double *>(a.cells)[at + j];
        } else if (a.elemType != 1) {
            const GfU4 c = *reinterpret_cast<const GfU4 *>(reinterpret_cast<const uint32_t *>(a.cells) + at);
            z[0] = cell_z(a, c.x), z[1] = cell_z(a, c.y), z[2] = cell_z(a, c.z), z[3] = cell_z(a, c.w);
        } else if (shortAligned) {
            const uint2 c = *reinterpret_cast<const uint2 *>(reinterpret_cast<const int16_t *>(a.cells) + at);
            z[0] = cell_z(a, (uint32_t)(int32_t)(int16_t)(c.x & 0xffffu)), z[1] = cell_z(a, (uint32_t)(int32_t)(int16_t)(c.x >> 16));
            z[2] = cell_z(a, (uint32_t)(int32_t)(int16_t)(c.y & 0xffffu)), z[3] = cell_z(a, (uint32_t)(int32_t)(int16_t)(c.y >> 16));
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) z[j] = cell_z(a, (uint32_t)(int32_t) reinterpret_cast<const int16_t *>(a.cells)[at + j]);
        }
        double sh[4] = {0.0, 0.0, 0.0, 0.0};
        if (withShade) {
#pragma unroll
            for (int j = 0; j < 4; j++) sh[j] = a.shade[at + j];
        }
        uint4 o;
        o.x = palette_argb(a.pal, z[0], sh[0], withShade);
        o.y = palette_argb(a.pal, z[1], sh[1], withShade);
        o.z = palette_argb(a.pal, z[2], sh[2], withShade);
        o.w = palette_argb(a.pal, z[3], sh[3], withShade);
        *reinterpret_cast<uint4 *>(a.argb + at) = o;
    }
}

// what a pixel stores: the words asked for, each exactly once
__device__ __forceinline__ void store_pixel(const GfRenderArgs &a, size_t t, const GfInterpResult &res, int status)
{
    double shade = 0.0;
    if (a.lit) shade = gf_render_shade(res.zx, res.zy, a.light);
    if (a.argb) a.argb[t] = palette_argb(a.pal, res.z, shade, a.lit != 0);
    if (a.shade) a.shade[t] = shade;
    if (a.status) a.status[t] = status;
}

// ------------------------------------------------------------------------------------------------
// k_render_points: a lane per point, as k_interp_points: a point list, or a lattice with a column spacing per row.  The point goes
// through gf_interp_point; a point without a result has NaN z, zx and zy, which the shade turns into the ambient level and the
// lookup into the null colour: no case of its own.
// ------------------------------------------------------------------------------------------------
template <bool LATTICE>
__global__ __launch_bounds__(RD_THREADS) void k_render_points(const GfRenderArgs a, const size_t first, const size_t end)
{
    stage_palette(a.pal);
    __syncthreads();
    const GfInterpArgs &ip = a.ip;
    const size_t t0 = first + ((size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x) * RD_THREADS;     // (workgroup-uniform)
    const size_t t = t0 + threadIdx.x;
    if (t >= end) return;
    double row, col, cs = ip.g.colSpacing;
    if (LATTICE) {
        // (i, j) of point t, as k_interp_points finds them
        const size_t i0 = t0 / ip.latCols, jj = t0 - i0 * ip.latCols + threadIdx.x;
        const size_t q = ip.latCols >= RD_THREADS ? (size_t)(jj >= ip.latCols) : (size_t)((uint32_t)jj / (uint32_t)ip.latCols);
        const size_t i = i0 + q, j = jj - q * ip.latCols;
        row = ip.latRow0 + (double)i * ip.latRowStep;
        col = ip.latCol0 + (double)j * ip.latColStep;
        if (ip.colSpacing) cs = ip.colSpacing[i];
    } else {
        row = ip.rows[t];
        col = ip.cols[t];
        if (ip.colSpacing) cs = ip.colSpacing[t];
    }
    GfInterpResult r;
    const int status = gf_interp_point(ip.g, ip.block, row, col, cs, false, r);
    store_pixel(a, t, r, status);
}

// ------------------------------------------------------------------------------------------------
// k_render_lattice: the fused kernel for a lattice with ONE column spacing, on the patch scheme of k_interp_lattice: a workgroup per
// patch of RL_ROWS x RL_COLS pixels; what depends on the column alone once per patch by the lanes of wave 0, what depends on the row
// alone by the first lanes of wave 1, through the functions the interpolator's kernels call; both in LDS (64 x 112 + 16 x 112
// bytes), the palette beside them.  Lane l of wave w takes column l of the patch and rows w, w + 4, ...: sixteen samples, the sums,
// the shade, the lookup, one 4-byte store; a wave's stores are 256 consecutive bytes of an image row.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t RL_ROWS = 16, RL_COLS = 64;

struct RlAxis {                        // 112 bytes
    GfInterpBasis B;
    int32_t at, n1, status, pad;       // row0 / col0 of the window, the columns before the wrap, GF_IP_*
};

__global__ __launch_bounds__(RD_THREADS) void k_render_lattice(const GfRenderArgs a, const size_t patchCols)
{
    __shared__ RlAxis sCol[RL_COLS], sRow[RL_ROWS];
    const GfInterpArgs &ip = a.ip;
    const size_t w = (size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x;
    const size_t pr = w / patchCols, pc = w - pr * patchCols;
    const size_t i0 = pr * RL_ROWS, j0 = pc * RL_COLS;
    if (i0 >= ip.latRows) return;                                              // (the grid's padding; workgroup-uniform)
    const uint32_t tid = threadIdx.x;
    stage_palette(a.pal);
    if (tid < RL_COLS) {
        RlAxis x;
        double u = 0;
        x.at = 0, x.n1 = 4, x.pad = 0;
        x.status = gf_interp_window_col(ip.g, ip.latCol0 + (double)(j0 + tid) * ip.latColStep, x.at, x.n1, u);
        if (x.status == GF_IP_OK) gf_interp_basis(u, ip.g.colSpacing, ip.g.target, x.B);
        sCol[tid] = x;
    } else if (tid < RL_COLS + RL_ROWS) {
        RlAxis x;
        double v = 0;
        x.at = 0, x.n1 = 4, x.pad = 0;
        x.status = gf_interp_window_row(ip.g, ip.latRow0 + (double)(i0 + (tid - RL_COLS)) * ip.latRowStep, x.at, v);
        if (x.status == GF_IP_OK) gf_interp_basis(v, ip.g.rowSpacing, ip.g.target, x.B);
        sRow[tid - RL_COLS] = x;
    }
    __syncthreads();
    const size_t j = j0 + (tid & (RL_COLS - 1));
    if (j >= ip.latCols) return;
    const RlAxis c = sCol[tid & (RL_COLS - 1)];
#pragma unroll 1
    for (uint32_t r = tid / RL_COLS; r < RL_ROWS && i0 + r < ip.latRows; r += RD_THREADS / RL_COLS) {
        const size_t t = (i0 + r) * ip.latCols + j;
        GfInterpResult res;
        gf_interp_nullify(res);
        int status = gf_interp_window_status(sRow[r].status, c.status);
        if (status == GF_IP_OK && !gf_interp_window_in_block(ip.g, sRow[r].at, c.at, c.n1)) status = GF_IP_ERR_BOUNDS;
        if (status == GF_IP_OK) {
            double z[16];
            gf_interp_samples(ip.g, ip.block, sRow[r].at, c.at, c.n1, z);
            gf_interp_sums(z, c.B, sRow[r].B, ip.g.target, res);
        }
        store_pixel(a, t, res, status);
    }
}

size_t paletteLds(const GfRenderPal &p) { return (size_t)80 * (size_t)p.head.n; }

}  // namespace

hipError_t gf_launch_render_cells(const GfRenderCellsArgs &a, hipStream_t stream)
{
    if (!a.cells || !a.argb || !a.pal.table || a.pal.head.n < 1 || a.pal.head.n > GF_PAL_MAX_RECORDS) return hipErrorInvalidValue;
    if (a.nCells == 0) return hipSuccess;
    size_t head = ((16 - ((uintptr_t)a.argb & 15u)) & 15u) / 4;
    if (head > a.nCells) head = a.nCells;
    const size_t nGroups = (a.nCells - head) / 4;
    const size_t perWg = (size_t)RC_ITERS * RD_THREADS;
    const size_t nWg = nGroups ? (nGroups + perWg - 1) / perWg : 1;
    if (nWg > ((size_t)1 << 20) * 65535u) return hipErrorInvalidValue;        // (2^48 cells)
    hipLaunchKernelGGL(k_render_cells, gf_tile_grid(nWg), dim3(RD_THREADS), paletteLds(a.pal), stream, a, (uint32_t)head, nGroups);
    return hipGetLastError();
}

hipError_t gf_launch_render(const GfRenderArgs &a, hipStream_t stream)
{
    const GfInterpArgs &ip = a.ip;
    if (!ip.block || (!a.argb && !a.shade) || (!ip.rows && (ip.latCols == 0 || ip.latRows == 0))) return hipErrorInvalidValue;
    if (!a.pal.table || a.pal.head.n < 1 || a.pal.head.n > GF_PAL_MAX_RECORDS) return hipErrorInvalidValue;
    const size_t lds = paletteLds(a.pal);
    if (!ip.rows && !ip.colSpacing) {
        const size_t patchRows = (ip.latRows + RL_ROWS - 1) / RL_ROWS, patchCols = (ip.latCols + RL_COLS - 1) / RL_COLS;
        if (patchRows <= (((size_t)1 << 20) * 65535u) / patchCols) {
            hipLaunchKernelGGL(k_render_lattice, gf_tile_grid(patchRows * patchCols), dim3(RD_THREADS), lds, stream, a, patchCols);
            return hipGetLastError();
        }
    }
    constexpr size_t perLaunch = ((size_t)1 << 20) * 65535u * RD_THREADS;
    for (size_t first = 0; first < ip.nPoints; first += perLaunch) {
        const size_t n = ip.nPoints - first < perLaunch ? ip.nPoints - first : perLaunch;
        const dim3 grid = gf_tile_grid((n + RD_THREADS - 1) / RD_THREADS);
        if (ip.rows) hipLaunchKernelGGL(k_render_points<false>, grid, dim3(RD_THREADS), lds, stream, a, first, first + n);
        else hipLaunchKernelGGL(k_render_points<true>, grid, dim3(RD_THREADS), lds, stream, a, first, first + n);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
