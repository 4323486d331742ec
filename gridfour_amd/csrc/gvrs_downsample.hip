// gvrs_downsample.hip -- a grid block in device memory averaged down by an integer factor f: output cell (i, j) is the box average of
// the f x f source cells behind it, bit for bit what the reference's ExampleDownsample computes cell by cell
// (demo/src/main/java/org/gridfour/demo/globalDEM/ExampleDownsample.java:164-210).  The arithmetic is gvrs_downsample_common.h,
// shared with the CPU harness; this file is the data path.  Per output cell: f * f loads, one store, almost no arithmetic.
//
// k_downsample_direct, a lane per output cell, consecutive lanes on consecutive output columns of one output row: a wave's loads
// of one source row cover one contiguous run of 64 * f cells.  F > 0: the factor is a compile-time constant (1 .. 8) and the
// window's loads are all issued before the first addition.  VEC: one load of f cells per lane and row (8 / 16 bytes for f = 2 / 4
// of 4-byte cells, 4 / 8 / 16 bytes for f = 2 / 4 / 8 of SHORT cells); whether pointer, column phase and row pitch allow it is
// decided per launch on the host.  F == 0: any factor, scalar loads in two loops.
//
// k_downsample_staged, for the factors at which a stride of f cells between lanes wastes the memory system: a workgroup takes W
// consecutive cells of one output row (W * f <= DS_LDS_CELLS), loads strips of source rows with lane-contiguous loads into LDS --
// one dword per cell, a pad dword after every 32, so that lanes f dwords apart do not meet on a bank -- and lane l < W then sums
// the cells of its window from LDS, rows in order and the cells of a row in order: the float chain is the reference's.  A window
// wider than the LDS (f > DS_LDS_CELLS) is one cell per workgroup walked in column chunks, the running sum carried in the lane.
//
// Every output cell is written exactly once; nothing outside the block is read.

#include <hip/hip_runtime.h>

#include <type_traits>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_downsample_common.h"
#include "gvrs_image_common.h"

namespace {

constexpr uint32_t DS_THREADS = 256;
constexpr uint32_t DS_LDS_CELLS = 4096;            // cells of a stage (16.5 KiB with the pad dwords: nine workgroups per CU)
constexpr uint32_t DS_STAGE_LOADS = 8;             // loads a lane has in flight while a stage fills

// the window's accumulator of an element type
template <typename T>
struct DsAcc {
    GfDsIntAcc a;
    __device__ void start() { gf_ds_int_start(a); }
    __device__ void add(T v, int32_t fill) { gf_ds_int_add(a, (int32_t)v, fill); }
    __device__ T finish(int32_t fill, int32_t n) const { return (T)gf_ds_int_finish(a, fill, n); }
};
template <>
struct DsAcc<float> {
    float sum;
    __device__ void start() { gf_ds_float_start(sum); }
    __device__ void add(float v, int32_t) { gf_ds_float_add(sum, v); }
    __device__ float finish(int32_t, int32_t n) const { return gf_ds_float_finish(sum, n); }
};

// a packed ARGB word as a cell type of its own (g.elemType GF_DS_ARGB): the channels are summed apart and the finish is
// makeReducedImage's (gvrs_image_common.h); there is no fill
struct DsArgb {
    uint32_t w;
    DsArgb() = default;
    __device__ explicit DsArgb(uint32_t bits) : w(bits) {}
};
template <>
struct DsAcc<DsArgb> {
    GfImgAcc a;
    __device__ void start() { gf_img_acc_start(a); }
    __device__ void add(DsArgb v, int32_t) { gf_img_acc_add(a, v.w); }
    __device__ DsArgb finish(int32_t, int32_t n) const { return DsArgb(gf_img_acc_finish(a, n)); }
};

// a cell as the dword an LDS stage holds, and back
template <typename T>
__device__ __forceinline__ uint32_t dsBits(T v)
{
    if constexpr (std::is_same_v<T, float>) return __float_as_uint(v);
    else if constexpr (std::is_same_v<T, DsArgb>) return v.w;
    else return (uint32_t)(int32_t)v;
}
template <typename T>
__device__ __forceinline__ T dsCell(uint32_t bits)
{
    if constexpr (std::is_same_v<T, float>) return __uint_as_float(bits);
    else if constexpr (std::is_same_v<T, DsArgb>) return DsArgb(bits);
    else return (T)(int32_t)bits;
}

// BYTES of a row of a window in one load
template <int BYTES>
struct alignas(BYTES) DsWords {
    uint32_t w[BYTES / 4];
};
template <typename T, int BYTES>
__device__ __forceinline__ T dsCellOf(const DsWords<BYTES> &v, int c)
{
    if constexpr (sizeof(T) == 2) return (T)(int16_t)(uint16_t)(v.w[c >> 1] >> (16 * (c & 1)));
    else return dsCell<T>(v.w[c]);
}

// the workgroup's output row and first column: one 64-bit division per workgroup
struct DsPlace {
    size_t i, group;
};
__device__ __forceinline__ DsPlace dsPlace(size_t wg0, size_t colGroups)
{
    const size_t w = wg0 + (size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x;
    const size_t i = w / colGroups;
    return {i, w - i * colGroups};
}

template <typename T, int F, bool VEC>
__global__ __launch_bounds__(DS_THREADS) void k_downsample_direct(const GfDsGeom g, const T *__restrict__ block, T *__restrict__ out,
                                                                  const size_t colGroups, const size_t wg0)
{
    const DsPlace at = dsPlace(wg0, colGroups);
    if (at.i >= (size_t)g.outRows) return;                                     // (the grid's padding; workgroup-uniform)
    const size_t j = at.group * DS_THREADS + threadIdx.x;
    if (j >= (size_t)g.outCols) return;
    const int32_t f = F ? F : g.f;
    const T *p = block + ((size_t)g.rowOff + at.i * (size_t)f) * (size_t)g.pitch + (size_t)g.colOff + j * (size_t)f;
    DsAcc<T> acc;
    acc.start();
    if constexpr (F > 0) {
        T v[F][F];
#pragma unroll
        for (int r = 0; r < F; r++) {
            const T *row = p + (size_t)r * (size_t)g.pitch;
            if constexpr (VEC) {
                const DsWords<F * (int)sizeof(T)> x = *reinterpret_cast<const DsWords<F * (int)sizeof(T)> *>(row);
#pragma unroll
                for (int c = 0; c < F; c++) v[r][c] = dsCellOf<T>(x, c);
            } else {
#pragma unroll
                for (int c = 0; c < F; c++) v[r][c] = row[c];
            }
        }
#pragma unroll
        for (int r = 0; r < F; r++)
#pragma unroll
            for (int c = 0; c < F; c++) acc.add(v[r][c], g.fillI);
    } else {
        for (int32_t r = 0; r < f; r++, p += g.pitch)
            for (int32_t c = 0; c < f; c++) acc.add(p[c], g.fillI);
    }
    out[at.i * (size_t)g.outCols + j] = acc.finish(g.fillI, f * f);
}

__device__ __forceinline__ uint32_t dsPad(uint32_t x) { return x + (x >> 5); }

// perGroup: output cells of a workgroup (W); chunk: cells per lane and row of a stage (f, or DS_LDS_CELLS when f is larger and
// perGroup is 1); rowsPer: source rows of a stage (1 when chunk < f, so that the chunks of a row stay in order)
template <typename T>
__global__ __launch_bounds__(DS_THREADS) void k_downsample_staged(const GfDsGeom g, const T *__restrict__ block, T *__restrict__ out,
                                                                  const uint32_t perGroup, const uint32_t chunk, const uint32_t rowsPer,
                                                                  const size_t colGroups, const size_t wg0)
{
    __shared__ uint32_t s[DS_LDS_CELLS + DS_LDS_CELLS / 32];
    const DsPlace at = dsPlace(wg0, colGroups);
    if (at.i >= (size_t)g.outRows) return;                                     // (workgroup-uniform)
    const size_t j0 = at.group * perGroup;
    const uint32_t nj = (size_t)g.outCols - j0 < perGroup ? (uint32_t)((size_t)g.outCols - j0) : perGroup;
    const uint32_t tid = threadIdx.x, f = (uint32_t)g.f;
    const T *src = block + ((size_t)g.rowOff + at.i * (size_t)f) * (size_t)g.pitch + (size_t)g.colOff + j0 * (size_t)f;
    DsAcc<T> acc;
    acc.start();
    for (uint32_t r0 = 0; r0 < f; r0 += rowsPer) {
        const uint32_t nr = f - r0 < rowsPer ? f - r0 : rowsPer;
        for (uint32_t c0 = 0; c0 < f; c0 += chunk) {                           // (one trip unless the window is wider than the LDS)
            const uint32_t n = f - c0 < chunk ? f - c0 : chunk;                // cells per lane and row
            const uint32_t run = nj * n;                                       // contiguous cells per source row: n == f, or nj == 1
            const uint32_t trips = (run + DS_THREADS - 1) / DS_THREADS, slots = nr * trips;
            for (uint32_t k0 = 0; k0 < slots; k0 += DS_STAGE_LOADS) {
                T v[DS_STAGE_LOADS];
                uint32_t to[DS_STAGE_LOADS];
#pragma unroll
                for (uint32_t u = 0; u < DS_STAGE_LOADS; u++) {
                    const uint32_t k = k0 + u, rr = k / trips, x = (k - rr * trips) * DS_THREADS + tid;
                    const bool ok = k < slots && x < run;
                    to[u] = ok ? dsPad(rr * run + x) : ~0u;
                    v[u] = ok ? src[(size_t)(r0 + rr) * (size_t)g.pitch + c0 + x] : T(0);
                }
#pragma unroll
                for (uint32_t u = 0; u < DS_STAGE_LOADS; u++)
                    if (to[u] != ~0u) s[to[u]] = dsBits<T>(v[u]);
            }
            __syncthreads();
            if (tid < nj)
                for (uint32_t rr = 0; rr < nr; rr++) {
                    const uint32_t base = rr * run + tid * n;
                    for (uint32_t c = 0; c < n; c++) acc.add(dsCell<T>(s[dsPad(base + c)]), g.fillI);
                }
            __syncthreads();
        }
    }
    if (tid < nj) out[at.i * (size_t)g.outCols + j0 + tid] = acc.finish(g.fillI, (int32_t)(f * f));
}

// workgroups of a call, a few launches at most (one in practice)
template <class Launch>
hipError_t dsLaunches(size_t nGroups, Launch launch)
{
    constexpr size_t perLaunch = ((size_t)1 << 20) * 65535u;
    for (size_t wg0 = 0; wg0 < nGroups; wg0 += perLaunch) {
        launch(gf_tile_grid(nGroups - wg0 < perLaunch ? nGroups - wg0 : perLaunch), wg0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename T, int F, bool VEC>
hipError_t dsDirect(const GfDownsampleArgs &a, hipStream_t stream)
{
    const size_t colGroups = ((size_t)a.g.outCols + DS_THREADS - 1) / DS_THREADS;
    return dsLaunches(colGroups * (size_t)a.g.outRows, [&](dim3 grid, size_t wg0) {
        hipLaunchKernelGGL((k_downsample_direct<T, F, VEC>), grid, dim3(DS_THREADS), 0, stream, a.g, (const T *)a.block, (T *)a.out, colGroups, wg0);
    });
}

// a window's row in one load: f cells are 4, 8 or 16 bytes and every row of every window starts on a multiple of that
template <typename T>
bool dsVecOk(const GfDownsampleArgs &a)
{
    const size_t bytes = (size_t)a.g.f * sizeof(T);
    if (bytes != 4 && bytes != 8 && bytes != 16) return false;
    if (sizeof(T) == 4 && bytes == 4) return false;                            // (f == 1: the scalar load is that load)
    return ((uintptr_t)a.block + (size_t)a.g.colOff * sizeof(T)) % bytes == 0 && ((size_t)a.g.pitch * sizeof(T)) % bytes == 0;
}

template <typename T>
hipError_t dsDirectAny(const GfDownsampleArgs &a, hipStream_t stream)
{
    if (dsVecOk<T>(a)) {
        if (a.g.f == 2) return dsDirect<T, 2, true>(a, stream);
        if (a.g.f == 4) return dsDirect<T, 4, true>(a, stream);
        if constexpr (sizeof(T) == 2)
            if (a.g.f == 8) return dsDirect<T, 8, true>(a, stream);
    }
    switch (a.g.f) {
    case 1: return dsDirect<T, 1, false>(a, stream);
    case 2: return dsDirect<T, 2, false>(a, stream);
    case 3: return dsDirect<T, 3, false>(a, stream);
    case 4: return dsDirect<T, 4, false>(a, stream);
    case 5: return dsDirect<T, 5, false>(a, stream);
    case 6: return dsDirect<T, 6, false>(a, stream);
    case 7: return dsDirect<T, 7, false>(a, stream);
    case 8: return dsDirect<T, 8, false>(a, stream);
    default: return dsDirect<T, 0, false>(a, stream);
    }
}

template <typename T>
hipError_t dsStaged(const GfDownsampleArgs &a, hipStream_t stream)
{
    const uint32_t f = (uint32_t)a.g.f;
    const uint32_t perGroup = f >= DS_LDS_CELLS ? 1 : std::min(DS_THREADS, DS_LDS_CELLS / f);
    const uint32_t chunk = std::min(f, DS_LDS_CELLS);
    const uint32_t rowsPer = chunk < f ? 1 : std::min(f, DS_LDS_CELLS / (perGroup * chunk));
    const size_t colGroups = ((size_t)a.g.outCols + perGroup - 1) / perGroup;
    return dsLaunches(colGroups * (size_t)a.g.outRows, [&](dim3 grid, size_t wg0) {
        hipLaunchKernelGGL((k_downsample_staged<T>), grid, dim3(DS_THREADS), 0, stream, a.g, (const T *)a.block, (T *)a.out, perGroup, chunk, rowsPer,
                           colGroups, wg0);
    });
}

template <typename T>
hipError_t dsAny(const GfDownsampleArgs &a, int path, hipStream_t stream)
{
    return path == GF_DS_STAGED ? dsStaged<T>(a, stream) : dsDirectAny<T>(a, stream);
}

}  // namespace

int gf_downsample_path(const GfDownsampleArgs &a)
{
    return a.g.f > GF_DS_DIRECT_MAX_FACTOR ? GF_DS_STAGED : GF_DS_DIRECT;
}

hipError_t gf_launch_downsample(const GfDownsampleArgs &a, int path, hipStream_t stream)
{
    if (!a.block || !a.out || a.g.f < 1 || a.g.outRows < 1 || a.g.outCols < 1) return hipErrorInvalidValue;
    if (path == GF_DS_AUTO) path = gf_downsample_path(a);
    switch (a.g.elemType) {
    case 0: return dsAny<int32_t>(a, path, stream);
    case 1: return dsAny<int16_t>(a, path, stream);
    case 2: return dsAny<float>(a, path, stream);
    case GF_DS_ARGB: return dsAny<DsArgb>(a, path, stream);
    default: return hipErrorInvalidValue;
    }
}
