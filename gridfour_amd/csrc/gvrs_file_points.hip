// gvrs_file_points.hip -- a GVRS file image read at scattered points: which tiles a set of points touches (k_points_mark,
// k_points_rank), and the decoded tiles sampled without a block in between (k_points_cells: GvrsElement.readValue /
// readValueInt, gvrs/GvrsElement.java; k_points_interp: GvrsInterpolatorBSpline.z / zNormal, gvrs/GvrsInterpolatorBSpline.java:
// 283-334), in the order in which gvrs_api_file_points.hip launches them around k_file_locate (gvrs_file.hip) and the records'
// pipeline (gvrs_records.hip), which runs untouched.  The arithmetic is gvrs_file_points.h and gvrs_interp_common.h, shared with
// the host forms and the CPU program; this file is the data path.  Built with -ffp-contract=off like the interpolation kernels.
// k_points_mark<true> and k_points_interp have a second instantiation each for points given at longitude / latitude or model
// x / y (GvrsInterpolatorBSpline.z / zNormal, :166-248): the mapping of gvrs_coords.h in registers, then the same body.

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_file_points.h"

namespace {

constexpr uint32_t PT_THREADS = 256;

// the OR over the wave's lanes, in every lane (all 64 lanes run it)
__device__ __forceinline__ uint32_t wave_or(uint32_t v)
{
    v |= gf_lane_xor(v, 1);
    v |= gf_lane_xor(v, 2);
    v |= gf_lane_xor(v, 4);
    v |= gf_lane_xor(v, 8);
    v |= gf_lane_xor(v, 16);
    v |= gf_lane_xor(v, 32);
    return v;
}

// One step of the marking: every lane of the wave runs it, a lane that `has` a tile brings its bitmap word w and bit m.  Points
// cluster -- a track's neighbours share a tile -- so the lanes that hold the same word are served together: the first pending
// lane's word is broadcast, its group's bits are ORed over the wave and the group's leader issues ONE atomicOr, and none where
// the word already holds the bits (a plain load: bits are only ever set, so a set bit read is a set bit).
__device__ __forceinline__ void mark_step(uint32_t *__restrict__ bits, bool has, uint32_t w, uint32_t m)
{
    bool pending = has;
    while (true) {
        const uint64_t todo = __ballot(pending);
        if (todo == 0) break;                                                  // (wave-uniform)
        uint32_t lw = 0;
        if (pending) lw = (uint32_t)__builtin_amdgcn_readfirstlane((int)w);    // the first pending lane's word
        const bool mine = pending && w == lw;
        const uint32_t group = wave_or(mine ? m : 0u);
        if (mine) {
            if ((uint32_t)__lane_id() == (uint32_t)(__ffsll((unsigned long long)todo) - 1)) {
                if ((bits[lw] & group) != group) atomicOr(bits + lw, group);
            }
            pending = false;
        }
    }
}

// WHERE POINT t OF A CALL LIES, for k_points_mark<true> and k_points_interp: its grid coordinates and column spacing, or
// GF_IP_ERR_ARG for a point refused before its window is looked at.  PtGiven: rows and columns as the call brought them.
// PtMapped: (a[t], b[t]) mapped in registers by gf_coords_query (gvrs_coords.h) -- the one function both kernels call, so they
// cannot disagree about a point's window; the mark kernel asks for no spacing and the cosine falls away there.
struct PtGiven {
    using MarkArgs = GfPointsMarkArgs;
    using InterpArgs = GfPointsInterpArgs;
    static __device__ __forceinline__ const GfPointsMarkArgs &mark(const MarkArgs &A) { return A; }
    static __device__ __forceinline__ const GfPointsInterpArgs &interp(const InterpArgs &A) { return A; }
    static __device__ __forceinline__ int at(const MarkArgs &A, size_t t, GfCoordsQuery &q)
    {
        q.row = A.rowsD[t], q.col = A.colsD[t], q.spacing = 0;
        return GF_IP_OK;
    }
    static __device__ __forceinline__ int at(const InterpArgs &A, size_t t, GfCoordsQuery &q)
    {
        q.row = A.rows[t], q.col = A.cols[t], q.spacing = A.colSpacing ? A.colSpacing[t] : A.ig.colSpacing;
        return GF_IP_OK;
    }
    static __device__ __forceinline__ void used(const InterpArgs &, size_t, double) {}
};
struct PtMapped {
    using MarkArgs = GfPointsMarkCoordsArgs;
    using InterpArgs = GfPointsInterpCoordsArgs;
    static __device__ __forceinline__ const GfPointsMarkArgs &mark(const MarkArgs &A) { return A.m; }
    static __device__ __forceinline__ const GfPointsInterpArgs &interp(const InterpArgs &A) { return A.p; }
    static __device__ __forceinline__ int at(const MarkArgs &A, size_t t, GfCoordsQuery &q)
    {
        return gf_coords_query(A.c, A.kind, A.m.rowsD[t], A.m.colsD[t], 0.0, false, q);
    }
    static __device__ __forceinline__ int at(const InterpArgs &A, size_t t, GfCoordsQuery &q)
    {
        const bool rule = A.p.colSpacing == nullptr;                           // (uniform)
        const int s = gf_coords_query(A.c, A.kind, A.p.rows[t], A.p.cols[t], A.p.ig.colSpacing, rule, q);
        if (!rule && s == GF_IP_OK) q.spacing = A.p.colSpacing[t];
        return s;
    }
    static __device__ __forceinline__ void used(const InterpArgs &A, size_t t, double spacing)   // (NaN for a refused point)
    {
        if (A.colSpacingUsed) A.colSpacingUsed[t] = spacing;
    }
};

// ------------------------------------------------------------------------------------------------
// k_points_mark: a lane per point, grid-stride in whole waves (the loop's trip count is wave-uniform: mark_step needs every lane).
// WINDOWS false: int32 cells, one tile each (gf_points_cell); true: double coordinates, the tiles of the 4 x 4 window
// (gf_interp_window, gf_points_window_tiles), one tile per step.  A refused point has no tile and marks nothing.  Where (windows
// only): PtGiven, the coordinates are the grid's; PtMapped, they are mapped first.
// ------------------------------------------------------------------------------------------------
template <bool WINDOWS, class Where = PtGiven>
__global__ __launch_bounds__(PT_THREADS) void k_points_mark(const typename Where::MarkArgs A)
{
    const GfPointsMarkArgs &a = Where::mark(A);
    const size_t stride = (size_t)gridDim.x * PT_THREADS;
    for (size_t base = (size_t)blockIdx.x * PT_THREADS + (threadIdx.x & ~63u); base < a.nPoints; base += stride) {
        const size_t t = base + (threadIdx.x & 63u);
        const bool live = t < a.nPoints;
        if (!WINDOWS) {
            int32_t tile = 0, at = 0;
            const bool has = live && gf_points_cell(a.g, a.rowsI[t], a.colsI[t], tile, at);
            mark_step(a.bits, has, (uint32_t)tile >> 5, 1u << ((uint32_t)tile & 31u));
        } else {
            GfWindowTiles wt{};
            int32_t n = 0;
            if (live) {
                GfCoordsQuery q;
                GfInterpWindow w;
                if (Where::at(A, t, q) == GF_IP_OK && gf_interp_window(a.ig, q.row, q.col, w) == GF_IP_OK) {
                    wt = gf_points_window_tiles(a.g, w.row0, w.col0, w.n1);
                    n = wt.count();
                }
            }
            for (int32_t k = 0; __ballot(k < n) != 0; k++) {                   // (wave-uniform)
                const int32_t tile = k < n ? wt.at(k) : 0;
                mark_step(a.bits, k < n, (uint32_t)tile >> 5, 1u << ((uint32_t)tile & 31u));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_points_rank: ONE workgroup of GF_POINTS_RANK_CHUNK lanes walks the bitmap in chunks of as many words with a carried base: a
// lane per word, its popcount scanned over the wave (DPP) and over the 16 waves' totals in LDS.  prefix[w] = the touched tiles in
// front of word w; the lane then lists its word's tiles from that place on, in ascending order, as long as the place lies in front
// of maxTiles.  The grid has at most 2^27 tiles: 4,096 turns.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GF_POINTS_RANK_CHUNK) void k_points_rank(const GfPointsRankArgs a)
{
    __shared__ uint32_t sWave[GF_POINTS_RANK_CHUNK / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = gf_wave_id();
    uint32_t base = 0;
    for (uint32_t w0 = 0; w0 < a.nWords; w0 += GF_POINTS_RANK_CHUNK) {         // (workgroup-uniform)
        const uint32_t w = w0 + tid;
        uint32_t word = w < a.nWords ? a.bits[w] : 0u;
        const uint32_t pc = (uint32_t)__popc(word);
        const uint32_t incl = gf_wave_incl_scan(pc);
        if (lane == 63u) sWave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < GF_POINTS_RANK_CHUNK / 64; k++) {
            const uint32_t s = sWave[k];
            before += k < wave ? s : 0u;
            total += s;
        }
        uint32_t at = base + before + incl - pc;
        if (w < a.nWords) a.prefix[w] = at;
        while (word != 0u && at < a.maxTiles) {
            const uint32_t b = (uint32_t)__ffs((int)word) - 1u;
            a.list[at++] = (int32_t)(w * 32u + b);
            word &= word - 1u;
        }
        base += total;
        __syncthreads();                                                       // (sWave is written again in the next turn)
    }
    if (tid == 0) *a.count = base;
}

// what a tile's slot says: where its cells lie, whether they may be read, the element's status there.  A slot outside the list
// (the bitmap and the points disagree: cannot happen, and must not read behind the pool) is refused.
struct PtSlot {
    uint32_t slot;
    bool readable;
    int32_t status;
};
__device__ __forceinline__ PtSlot pt_slot(const GfPointsLookup &k, const int32_t *__restrict__ slotStatus, int32_t tile)
{
    PtSlot s;
    s.slot = gf_points_slot(k.bits, k.prefix, tile);
    if (s.slot >= k.nSlots) {
        s.slot = 0, s.readable = false, s.status = GF_K_ERR_BOUNDS;
        return s;
    }
    s.status = slotStatus[s.slot];
    s.readable = k.verdict[s.slot] == GF_FILE_LOCATED && s.status == GF_K_OK;
    return s;
}

// ------------------------------------------------------------------------------------------------
// k_points_cells: a lane per point.  The cell's tile and index in it once, then per element the slot's status and the one cell
// at slot * cells + indexInTile of the element's pool, or the fill where the tile has no record, was refused or the element did
// not decode.  A point outside the grid: GF_K_ERR_ARG and the fill for every element.  Loads of neighbouring points are
// neighbours where the points are; stores are coalesced: values[e][i], status[e * nPoints + i].
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PT_THREADS) void k_points_cells(const GfPointsCellsArgs a)
{
    const size_t t = ((size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x) * PT_THREADS + threadIdx.x;
    if (t >= a.nPoints) return;
    int32_t tile = 0, at = 0;
    const bool inGrid = gf_points_cell(a.g, a.rows[t], a.cols[t], tile, at);
    for (int e = 0; e < a.nElems; e++) {                                       // (uniform)
        const GfPointsElem d = a.elems[e];
        PtSlot s;
        s.slot = 0, s.readable = false, s.status = GF_K_ERR_ARG;
        if (inGrid) s = pt_slot(a.look, a.look.slotStatus + (size_t)e * a.look.nSlots, tile);
        const size_t cell = (size_t)s.slot * a.look.cells + (size_t)at;
        if (d.itemBytes == 2u) {
            uint16_t v = (uint16_t)d.fillBits;
            if (s.readable) v = reinterpret_cast<const uint16_t *>(d.pool)[cell];
            reinterpret_cast<uint16_t *>(d.values)[t] = v;
        } else {
            uint32_t v = d.fillBits;
            if (s.readable) v = reinterpret_cast<const uint32_t *>(d.pool)[cell];
            reinterpret_cast<uint32_t *>(d.values)[t] = v;
        }
        a.status[(size_t)e * a.nPoints + t] = s.status;
    }
}

// ------------------------------------------------------------------------------------------------
// k_points_interp: a lane per point.  gf_interp_point's steps with the block replaced by the pool: the window, the spacing check,
// the sixteen samples, gf_interp_basis / gf_interp_sums / gf_interp_unit_normal unchanged.  The window's rows and columns are
// walked once for their tiles (one division each: the next row or column is the same tile or the next one's first), a tile's slot
// is looked up when the walk enters it and kept for the columns of a tile row, and a sample is the cell's bits from the pool, or
// the fill's where the tile has none to read, converted exactly as gf_interp_samples converts a block's cell.  If the element of
// any tile of the window did not decode, the point takes the status of the lowest-indexed such tile and NaN.  Outputs are
// structure-of-arrays; every item is written exactly once.  No LDS, no scratch.
// Where: PtGiven, the points in grid coordinates with the call's spacings; PtMapped, the points mapped first (a point the latitude
// check refuses is GF_K_ERR_ARG, in front of everything the window decides) and the spacing each was evaluated with stored.
// ------------------------------------------------------------------------------------------------
template <class Where>
__global__ __launch_bounds__(PT_THREADS) void k_points_interp(const typename Where::InterpArgs A)
{
    const GfPointsInterpArgs &a = Where::interp(A);
    const size_t t = ((size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x) * PT_THREADS + threadIdx.x;
    if (t >= a.nPoints) return;
    GfCoordsQuery q;
    const int refused = Where::at(A, t, q);
    const double row = q.row, col = q.col, cs = q.spacing;
    Where::used(A, t, cs);                                                     // (stored at once: one register pair less to carry)
    GfInterpResult res;
    gf_interp_nullify(res);
    GfInterpWindow w;
    int status = refused != GF_IP_OK ? refused : gf_interp_window(a.ig, row, col, w);
    if (status == GF_IP_OK && a.ig.target != GF_IP_VALUE && (cs == 0 || a.ig.rowSpacing == 0)) status = GF_IP_ERR_ARG;
    if (status == GF_IP_OK) {
        const int32_t nRT = a.g.nRowsTile, nCT = a.g.nColsTile;
        // the columns: tile column and column in the tile of sample k
        int32_t tc[4], inCol[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool first = k == 0 || k == w.n1;                            // a run begins
            if (first) {
                const int32_t c = gf_points_window_col(w.col0, w.n1, k);
                tc[k] = c / nCT, inCol[k] = c - tc[k] * nCT;
            } else {
                const bool next = inCol[k - 1] + 1 == nCT;
                tc[k] = tc[k - 1] + (next ? 1 : 0), inCol[k] = next ? 0 : inCol[k - 1] + 1;
            }
        }
        int32_t tr = w.row0 / nRT, inRow = w.row0 - tr * nRT;
        int32_t badTile = 0x7fffffff, badStatus = GF_K_OK;
        size_t cellBase[4];                                                    // per column: slot * cells of the tile row's tile, or ~0: fill
        uint32_t q[16];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (r > 0) {
                inRow++;
                if (inRow == nRT) inRow = 0, tr++;
            }
            if (r == 0 || inRow == 0) {                                        // the walk enters a tile row
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (k > 0 && tc[k] == tc[k - 1]) cellBase[k] = cellBase[k - 1];
                    else if (k > 0 && tc[k] == tc[0]) cellBase[k] = cellBase[0];
                    else {
                        const int32_t tile = tr * a.g.nColsOfTiles + tc[k];
                        const PtSlot s = pt_slot(a.look, a.look.slotStatus, tile);
                        cellBase[k] = s.readable ? (size_t)s.slot * a.look.cells : ~(size_t)0;
                        if (s.status != GF_K_OK && tile < badTile) badTile = tile, badStatus = s.status;
                    }
                }
            }
            const size_t rowAt = (size_t)inRow * (size_t)nCT;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t v = a.ig.elemType == 1 ? (uint32_t)(int32_t)(int16_t)a.fillBits : a.fillBits;
                if (cellBase[k] != ~(size_t)0) {
                    const size_t at = cellBase[k] + rowAt + (size_t)inCol[k];
                    v = a.ig.elemType != 1 ? reinterpret_cast<const uint32_t *>(a.pool)[at]
                                           : (uint32_t)(int32_t) reinterpret_cast<const int16_t *>(a.pool)[at];
                }
                q[4 * r + k] = v;
            }
        }
        if (badStatus != GF_K_OK) status = badStatus;
        else {
            double z[16];
#pragma unroll
            for (int i = 0; i < 16; i++) z[i] = a.ig.elemType >= 2 ? gf_interp_sample_f32(q[i]) : gf_interp_sample_i32((int32_t)q[i], a.ig.fillI);
            GfInterpBasis bu, pv;
            gf_interp_basis(w.u, cs, a.ig.target, bu);
            gf_interp_basis(w.v, a.ig.rowSpacing, a.ig.target, pv);
            gf_interp_sums(z, bu, pv, a.ig.target, res);
            if (a.normal) gf_interp_unit_normal(res.zx, res.zy, res.normal);
        }
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

}  // namespace

hipError_t gf_launch_points_mark(const GfPointsMarkArgs &a, bool windows, hipStream_t stream)
{
    if (a.nPoints == 0) return hipSuccess;
    if (a.nPoints > 0x7fffffffull || !a.bits || a.g.nTilesGrid < 1) return hipErrorInvalidValue;
    if (windows ? (!a.rowsD || !a.colsD) : (!a.rowsI || !a.colsI)) return hipErrorInvalidValue;
    // grid-stride: enough workgroups to fill the device a few times over, no more than the points need
    const size_t need = (a.nPoints + PT_THREADS - 1) / PT_THREADS;
    const unsigned grid = (unsigned)(need < 4096 ? need : 4096);
    if (windows) hipLaunchKernelGGL(k_points_mark<true>, dim3(grid), dim3(PT_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(k_points_mark<false>, dim3(grid), dim3(PT_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_points_rank(const GfPointsRankArgs &a, hipStream_t stream)
{
    if (!a.bits || !a.prefix || !a.count || (a.maxTiles && !a.list) || a.nWords > (1u << 22)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_points_rank, dim3(1), dim3(GF_POINTS_RANK_CHUNK), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_points_cells(const GfPointsCellsArgs &a, hipStream_t stream)
{
    if (a.nPoints == 0) return hipSuccess;
    if (a.nElems < 1 || a.nElems > GF_K_MAX_ELEMS || !a.rows || !a.cols || !a.status) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_points_cells, gf_tile_grid((a.nPoints + PT_THREADS - 1) / PT_THREADS), dim3(PT_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_points_interp(const GfPointsInterpArgs &a, hipStream_t stream)
{
    if (a.nPoints == 0) return hipSuccess;
    if (!a.rows || !a.cols || !a.z) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_points_interp<PtGiven>, gf_tile_grid((a.nPoints + PT_THREADS - 1) / PT_THREADS), dim3(PT_THREADS), 0, stream, a);
    return hipGetLastError();
}

static bool coordsKind(int32_t kind) { return kind == GF_CO_GRID || kind == GF_CO_FILE; }

hipError_t gf_launch_points_mark_coords(const GfPointsMarkCoordsArgs &a, hipStream_t stream)
{
    if (a.m.nPoints == 0) return hipSuccess;
    if (a.m.nPoints > 0x7fffffffull || !a.m.bits || a.m.g.nTilesGrid < 1 || !a.m.rowsD || !a.m.colsD || !coordsKind(a.kind)) return hipErrorInvalidValue;
    const size_t need = (a.m.nPoints + PT_THREADS - 1) / PT_THREADS;           // (as gf_launch_points_mark)
    const unsigned grid = (unsigned)(need < 4096 ? need : 4096);
    hipLaunchKernelGGL((k_points_mark<true, PtMapped>), dim3(grid), dim3(PT_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_points_interp_coords(const GfPointsInterpCoordsArgs &a, hipStream_t stream)
{
    if (a.p.nPoints == 0) return hipSuccess;
    if (!a.p.rows || !a.p.cols || !a.p.z || !coordsKind(a.kind)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_points_interp<PtMapped>, gf_tile_grid((a.p.nPoints + PT_THREADS - 1) / PT_THREADS), dim3(PT_THREADS), 0, stream, a);
    return hipGetLastError();
}
