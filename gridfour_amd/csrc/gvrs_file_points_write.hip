// gvrs_file_points_write.hip -- a GVRS file image WRITTEN at scattered points: GvrsElement.writeValue / writeValueInt over a batch
// (gvrs/GvrsElement.java; the cell rule of TileElement*.setValue is gvrs_file_points_store.h, shared with the block write), in the
// order in which gvrs_api_file_points.hip launches the kernels around mark and rank (gvrs_file_points.hip), k_file_locate
// (gvrs_file.hip), the records' pipeline (gvrs_records.hip), the record writer (gvrs_records_enc.hip) and the update kernels
// (gvrs_file_update.hip), which all run untouched.  The reference stores the points one after the other; here "the last point
// whose value passed wins" is decided by the point INDEX, never by timing: k_points_claim raises a cell's owner word to the
// highest such index (atomicMax: the result is the maximum whatever the order), and only behind that launch k_points_store lets
// the owners write.  Built with -ffp-contract=off like every other source (the ICF conversion rounds twice in float32).

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_file_points.h"
#include "gvrs_file_points_store.h"
#include "gvrs_file_update.h"

namespace {

constexpr uint32_t PW_THREADS = 256;

__device__ __forceinline__ GfStoreElem pw_elem(const GfPointsWriteElem &d)
{
    return gf_store_elem(d.type, d.fillBits, d.fillFBits, d.minBits, d.maxBits, d.scale, d.offset);
}

// the value of point t as the cell rule takes it
__device__ __forceinline__ uint32_t pw_value(const GfPointsWriteElem &d, size_t t)
{
    return d.type == GF_K_ELEM_SHORT ? (uint32_t) reinterpret_cast<const uint16_t *>(d.values)[t] : reinterpret_cast<const uint32_t *>(d.values)[t];
}

// where a point's cell lies: false for a point outside the grid or a slot outside the list (the bitmap and the points disagree:
// cannot happen, and must not reach behind pool, planes or flags)
__device__ __forceinline__ bool pw_cell(const GfPointsWriteArgs &a, size_t t, uint32_t &slot, uint32_t &at, bool &inGrid)
{
    int32_t tile = 0, in = 0;
    inGrid = gf_points_cell(a.g, a.rows[t], a.cols[t], tile, in);
    slot = 0, at = 0;
    if (!inGrid) return false;
    slot = gf_points_slot(a.look.bits, a.look.prefix, tile);
    at = (uint32_t)in;
    return slot < a.look.nSlots && at < a.look.cells;
}

// ------------------------------------------------------------------------------------------------
// k_points_heads: a lane per slot, behind k_file_locate.  A located record's size and type words (one 8-byte load at its start,
// which k_file_locate found inside the image) are judged by the update's rule, gfFsHeadWords: a head it refuses becomes the
// slot's verdict and the slot gets the empty extent, which the framing walk refuses without reading anything.  So a tile the
// update could not free is never decoded, stored into or rewritten, and the host form's verdict (the same function) is this one.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PW_THREADS) void k_points_heads(const GfPointsHeadsArgs a)
{
    const uint32_t s = blockIdx.x * PW_THREADS + threadIdx.x;
    if (s >= a.nSlots || a.verdict[s] != GF_FILE_LOCATED) return;
    const uint64_t start = a.starts[s];                                       // (a multiple of 8 with start + 20 <= imageBytes: the place rule)
    const GfU2 h = *reinterpret_cast<const GfU2 *>(a.image + start);
    uint64_t size;
    const gf_status v = gfFsHeadWords(a.imageBytes, start + 8u, h.x, h.y, GF_FILE_REC_TILE, 24, &size);
    if (v != GF_OK) a.verdict[s] = (int32_t)v, a.starts[s] = 0, a.ends[s] = 0;
}

// ------------------------------------------------------------------------------------------------
// k_points_prepare: a workgroup per slot, behind the records' pipeline and k_file_status.  slotOld[s] = the first element status
// (element order) that is not GF_K_OK: the tile cannot be rewritten; stored[s] = 0; and for a tile the file holds no record of
// (the verdict GF_K_OK) every element's pool slot takes the fill, cells beyond the grid's edge included: the records' pipeline
// writes nothing into the slot of an empty extent.  A SHORT slot begins on a 2-byte boundary only: item by item.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PW_THREADS) void k_points_prepare(const GfPointsWriteArgs a)
{
    GF_FOR_WG_TILE(s, (size_t)a.look.nSlots)
    {
        if (threadIdx.x == 0) {
            int32_t st = GF_K_OK;
            for (int e = 0; e < a.nElems && st == GF_K_OK; e++) st = a.look.slotStatus[(size_t)e * a.look.nSlots + s];
            a.slotOld[s] = st;
            a.stored[s] = 0u;
        }
        if (a.look.verdict[s] != GF_K_OK) continue;                            // (workgroup-uniform) the file holds a record, or refuses
        const size_t base = s * (size_t)a.look.cells;
        for (int e = 0; e < a.nElems; e++) {                                   // (uniform)
            const GfPointsWriteElem d = a.elems[e];
            if (d.type == GF_K_ELEM_SHORT) {
                uint16_t *__restrict__ p = reinterpret_cast<uint16_t *>(d.pool) + base;
                for (uint32_t k = threadIdx.x; k < a.look.cells; k += PW_THREADS) p[k] = (uint16_t)d.fillBits;
            } else {
                uint32_t *__restrict__ p = reinterpret_cast<uint32_t *>(d.pool) + base;
                for (uint32_t k = threadIdx.x; k < a.look.cells; k += PW_THREADS) p[k] = d.fillBits;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_points_claim: a lane per point.  For a point of the grid whose tile can be rewritten, every element whose value passes the
// cell rule raises the cell's owner word to the point's index + 1.  Points are mostly distinct cells (a track, a scatter), so the
// lanes are not merged first: an atomic per passing (point, element), neighbours where the points are.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PW_THREADS) void k_points_claim(const GfPointsWriteArgs a)
{
    const size_t t = ((size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x) * PW_THREADS + threadIdx.x;
    if (t >= a.nPoints) return;
    uint32_t slot, at;
    bool inGrid;
    if (!pw_cell(a, t, slot, at, inGrid) || a.slotOld[slot] != GF_K_OK) return;
    const size_t cell = (size_t)slot * a.look.cells + at;
    for (int e = 0; e < a.nElems; e++) {                                       // (uniform)
        const GfPointsWriteElem d = a.elems[e];
        uint32_t o;
        if (gf_store_value_of(d.type, pw_value(d, t), pw_elem(d), o)) atomicMax(d.owner + cell, (uint32_t)t + 1u);
    }
}

// ------------------------------------------------------------------------------------------------
// k_points_store: a lane per point, behind k_points_claim.  The point's statuses, first match: GF_K_ERR_ARG for every element of
// a point outside the grid; the tile's status for every element where the tile cannot be rewritten; GF_K_ERR_BOUNDS for the
// element whose value the cell rule refuses; else GF_K_OK, and where the point owns the cell it stores the converted value (a
// SHORT's as two bytes).  A point with a passing value marks its tile as stored into, owner or not -- the reference's earlier
// store happened --: the lanes of a wave that share a tile are served together, ONE atomicOr per wave and tile, and none where
// the flag is already set.  Every lane of a wave runs the marking loop (threads beyond the points take part without a tile).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PW_THREADS) void k_points_store(const GfPointsWriteArgs a)
{
    const size_t t = ((size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x) * PW_THREADS + threadIdx.x;
    bool passed = false;
    uint32_t slot = 0;
    if (t < a.nPoints) {
        uint32_t at;
        bool inGrid;
        const bool has = pw_cell(a, t, slot, at, inGrid);
        const int32_t old = has ? a.slotOld[slot] : (inGrid ? GF_K_ERR_BOUNDS : GF_K_ERR_ARG);
        const size_t cell = (size_t)slot * a.look.cells + at;
        for (int e = 0; e < a.nElems; e++) {                                   // (uniform)
            const GfPointsWriteElem d = a.elems[e];
            int32_t st = old;
            if (has && old == GF_K_OK) {
                uint32_t o;
                if (!gf_store_value_of(d.type, pw_value(d, t), pw_elem(d), o)) st = GF_K_ERR_BOUNDS;
                else {
                    passed = true;
                    if (d.owner[cell] == (uint32_t)t + 1u) {
                        if (d.type == GF_K_ELEM_SHORT) reinterpret_cast<uint16_t *>(d.pool)[cell] = (uint16_t)o;
                        else reinterpret_cast<uint32_t *>(d.pool)[cell] = o;
                    }
                }
            }
            a.pointStatus[(size_t)e * a.nPoints + t] = st;
        }
    }
    bool pending = passed;
    while (true) {
        const uint64_t todo = __ballot(pending);
        if (todo == 0) break;                                                  // (wave-uniform)
        uint32_t first = 0;
        if (pending) first = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot);   // the first pending lane's slot
        if (pending && slot == first) {
            if ((uint32_t)__lane_id() == (uint32_t)(__ffsll((unsigned long long)todo) - 1)) {
                if (a.stored[first] == 0u) atomicOr(a.stored + first, 1u);
            }
            pending = false;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_points_verdict: a workgroup per touched tile, behind k_points_store.  tileIndices[s] = the tile, and preStatus[s], first
// match: the old record's status (the tile stays); GF_K_ERR_BOUNDS, no point stored anything (the reference never sets
// writingRequired: the tile stays); GF_K_DECLINED, no cell of any element is data after the stores (the record is freed); else 0
// and the record writer decides.  Only a tile that was stored into is scanned: its lanes stride over the cells of every element,
// a ballot per wave, and the waves' answers meet in LDS.  (A lane per tile would read a whole tile by itself, a cell per load
// and tiles apart: the scan is the workgroup's.)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PW_THREADS) void k_points_verdict(const GfPointsWriteArgs a)
{
    __shared__ uint32_t sValid;
    GF_FOR_WG_TILE(s, (size_t)a.look.nSlots)
    {
        const int32_t old = a.slotOld[s];
        const bool scan = old == GF_K_OK && a.stored[s] != 0u;                 // (workgroup-uniform)
        if (!scan) {
            if (threadIdx.x == 0) a.tileIndices[s] = a.list[s], a.preStatus[s] = old != GF_K_OK ? old : GF_K_ERR_BOUNDS;
            continue;
        }
        if (threadIdx.x == 0) sValid = 0u;
        __syncthreads();
        const size_t base = s * (size_t)a.look.cells;
        bool valid = false;
        for (int e = 0; e < a.nElems; e++) {                                   // (uniform)
            const GfPointsWriteElem d = a.elems[e];
            const GfStoreElem p = pw_elem(d);
            if (d.type == GF_K_ELEM_SHORT) {
                const uint16_t *__restrict__ q = reinterpret_cast<const uint16_t *>(d.pool) + base;
                for (uint32_t k = threadIdx.x; k < a.look.cells; k += PW_THREADS) valid |= gf_store_valid_of(d.type, q[k], p);
            } else {
                const uint32_t *__restrict__ q = reinterpret_cast<const uint32_t *>(d.pool) + base;
                for (uint32_t k = threadIdx.x; k < a.look.cells; k += PW_THREADS) valid |= gf_store_valid_of(d.type, q[k], p);
            }
        }
        if (__ballot(valid) != 0 && (threadIdx.x & 63u) == 0u) sValid = 1u;    // (every writer writes 1)
        __syncthreads();
        if (threadIdx.x == 0) a.tileIndices[s] = a.list[s], a.preStatus[s] = sValid ? 0 : GF_K_DECLINED;
    }
}

bool pwArgsOk(const GfPointsWriteArgs &a)
{
    if (a.nElems < 1 || a.nElems > GF_K_MAX_ELEMS || !a.look.bits || !a.look.prefix || !a.look.verdict || !a.look.slotStatus) return false;
    if (!a.slotOld || !a.stored || a.look.cells < 1) return false;
    for (int e = 0; e < a.nElems; e++)
        if (!a.elems[e].pool || !a.elems[e].owner || a.elems[e].type < GF_K_ELEM_INT || a.elems[e].type > GF_K_ELEM_ICF) return false;
    return true;
}

bool pwPointsOk(const GfPointsWriteArgs &a)
{
    if (!pwArgsOk(a) || a.nPoints > 0x7fffffffull || !a.rows || !a.cols || !a.pointStatus) return false;
    for (int e = 0; e < a.nElems; e++)
        if (!a.elems[e].values) return false;
    return true;
}

}  // namespace

hipError_t gf_launch_points_heads(const GfPointsHeadsArgs &a, hipStream_t stream)
{
    if (a.nSlots == 0) return hipSuccess;
    if (!a.image || ((uintptr_t)a.image & 7u) != 0 || !a.starts || !a.ends || !a.verdict || a.nSlots > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_points_heads, dim3((a.nSlots + PW_THREADS - 1) / PW_THREADS), dim3(PW_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_points_prepare(const GfPointsWriteArgs &a, hipStream_t stream)
{
    if (a.look.nSlots == 0) return hipSuccess;
    if (!pwArgsOk(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_points_prepare, gf_tile_grid(a.look.nSlots), dim3(PW_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_points_claim(const GfPointsWriteArgs &a, hipStream_t stream)
{
    if (a.nPoints == 0 || a.look.nSlots == 0) return hipSuccess;
    if (!pwPointsOk(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_points_claim, gf_tile_grid((a.nPoints + PW_THREADS - 1) / PW_THREADS), dim3(PW_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_points_store(const GfPointsWriteArgs &a, hipStream_t stream)
{
    if (a.nPoints == 0) return hipSuccess;
    if (!pwPointsOk(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_points_store, gf_tile_grid((a.nPoints + PW_THREADS - 1) / PW_THREADS), dim3(PW_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_points_verdict(const GfPointsWriteArgs &a, hipStream_t stream)
{
    if (a.look.nSlots == 0) return hipSuccess;
    if (!pwArgsOk(a) || !a.list || !a.tileIndices || !a.preStatus) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_points_verdict, gf_tile_grid(a.look.nSlots), dim3(PW_THREADS), 0, stream, a);
    return hipGetLastError();
}
