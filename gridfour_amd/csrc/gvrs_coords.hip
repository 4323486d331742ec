// gvrs_coords.hip -- k_coords_map: the coordinate mappings of a GVRS file over a batch of points (mapGeographicToGridPoint,
// mapModelToGridPoint with their GridPoint, mapGridToGeoPoint, mapGridToModelPoint: gvrs/GvrsFileSpecification.java:2101-2234;
// the column spacing of zNormal, gvrs/GvrsInterpolatorBSpline.java:226-232).  The arithmetic is gf_coords_map of gvrs_coords.h,
// shared with the host form (gvrs_api_coords.hip) and the CPU program; this file is the data path.  Built with -ffp-contract=off.

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_coords.h"

namespace {

constexpr uint32_t CO_THREADS = 256;

// ------------------------------------------------------------------------------------------------
// k_coords_map: a lane per point.  Two coalesced 8-byte loads, gf_coords_map in registers, one coalesced store per output array
// that was passed: the direction (kind) and the optional outputs are wave-uniform branches.  Every output item is written
// exactly once; t < nPoints bounds every access.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CO_THREADS) void k_coords_map(const GfCoordsMapArgs a)
{
    const size_t t = ((size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x) * CO_THREADS + threadIdx.x;
    if (t >= a.nPoints) return;
    GfCoordsMapped m;
    gf_coords_map(a.c, a.kind, a.a[t], a.b[t], m);
    a.outA[t] = m.outA;
    a.outB[t] = m.outB;
    if (a.kind == GF_CO_GRID_TO_GEO || a.kind == GF_CO_GRID_TO_MODEL) return;  // (uniform)
    if (a.iRow) a.iRow[t] = m.iRow;
    if (a.iCol) a.iCol[t] = m.iCol;
    if (a.colSpacing) a.colSpacing[t] = m.spacing;
    if (a.status) a.status[t] = m.status;
}

}  // namespace

hipError_t gf_launch_coords_map(const GfCoordsMapArgs &a, hipStream_t stream)
{
    if (a.nPoints == 0) return hipSuccess;
    if (a.kind < GF_CO_GEO_TO_GRID || a.kind > GF_CO_GRID_TO_MODEL || !a.a || !a.b || !a.outA || !a.outB) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_coords_map, gf_tile_grid((a.nPoints + CO_THREADS - 1) / CO_THREADS), dim3(CO_THREADS), 0, stream, a);
    return hipGetLastError();
}
