// gvrs_image.hip -- packed ARGB words split into three element planes and joined from them: the loops with which the reference's
// ExperimentalImageStorage stores an image as elements r, g, b or Y, Co, Cg and reads it back
// (demo/src/main/java/org/gridfour/demo/imaging/ExperimentalImageStorage.java:203-213, :242-256, :275-286).  The arithmetic is
// gvrs_image_common.h, shared with the CPU harness; this file is the data path: 4 bytes of words and 12 (INT planes) or 6 (SHORT
// planes) bytes of planes per pixel, almost no arithmetic.  The box average of packed words (gf_image_reduce_*) is not here: it
// runs through the two kernels of gvrs_downsample.hip with a packed-word accumulator.
//
// k_image_split / k_image_join, four pixels a lane: the words move as one 16-byte load / store per lane, a plane as one 16-byte
// (INT) or 8-byte (SHORT) store / load.  The bases are aligned to their items only, so the first `head` pixels (0 .. 3: up to the
// words' first 16-byte boundary) and the last `tail` (0 .. 3) go one by one, behind the quads in the same item space.  A plane
// whose phase differs from the words' -- (plane + head) is not on a boundary of its vector -- moves as four items a lane instead:
// decided per plane and launch on the host (vecMask), wave-uniform in the kernel.
// At most IMG_MAX_GROUPS workgroups, a grid-stride loop over size_t items.  Every output item is written exactly once; nothing
// outside the n_pixels items of any array is read or written.

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_image_common.h"

namespace {

constexpr uint32_t IMG_THREADS = 256;
constexpr uint32_t IMG_MAX_GROUPS = 2048;          // eight workgroups on each of 256 CUs; the stride loop takes the rest

struct alignas(16) ImgWords {
    uint32_t w[4];
};
// four items of a plane in one access: 16 bytes of int32, 8 bytes of int16
template <typename P>
struct alignas(4 * sizeof(P)) ImgQuad {
    P v[4];
};

template <typename P>
struct ImgPlanes {
    P *p[3];
};

// the item space of a launch: quads first, then the head's and the tail's single pixels
struct ImgSpan {
    size_t head, nQuads, tail;
    uint32_t vecMask;              // bit k: plane k moves as one vector per quad
};

__device__ __forceinline__ size_t imgSingle(const ImgSpan &s, size_t item)
{
    const size_t k = item - s.nQuads;
    return k < s.head ? k : s.head + 4 * s.nQuads + (k - s.head);
}

template <typename P, int MODEL>
__global__ __launch_bounds__(IMG_THREADS) void k_image_split(const uint32_t *__restrict__ argb, const ImgPlanes<P> planes, const ImgSpan s)
{
    const size_t nItems = s.nQuads + s.head + s.tail, stride = (size_t)gridDim.x * IMG_THREADS;
    for (size_t item = (size_t)blockIdx.x * IMG_THREADS + threadIdx.x; item < nItems; item += stride) {
        if (item < s.nQuads) {
            const size_t at = s.head + 4 * item;
            const ImgWords x = *reinterpret_cast<const ImgWords *>(argb + at);
            int32_t v[4][3];
#pragma unroll
            for (int i = 0; i < 4; i++) gf_img_split(MODEL, x.w[i], v[i]);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (s.vecMask >> k & 1u) {
                    typedef P QuadV __attribute__((ext_vector_type(4)));
                    const QuadV q = {(P)v[0][k], (P)v[1][k], (P)v[2][k], (P)v[3][k]};
                    __builtin_nontemporal_store(q, reinterpret_cast<QuadV *>(planes.p[k] + at));      // (written once, not read again here)
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) planes.p[k][at + i] = (P)v[i][k];
                }
            }
        } else {
            const size_t at = imgSingle(s, item);
            int32_t v[3];
            gf_img_split(MODEL, argb[at], v);
#pragma unroll
            for (int k = 0; k < 3; k++) planes.p[k][at] = (P)v[k];
        }
    }
}

// (P)v of an int16 plane sign-extends, as TileElementShort.getValueInt returns it
template <typename P, int MODEL>
__global__ __launch_bounds__(IMG_THREADS) void k_image_join(const ImgPlanes<const P> planes, uint32_t *__restrict__ argb, const ImgSpan s)
{
    const size_t nItems = s.nQuads + s.head + s.tail, stride = (size_t)gridDim.x * IMG_THREADS;
    for (size_t item = (size_t)blockIdx.x * IMG_THREADS + threadIdx.x; item < nItems; item += stride) {
        if (item < s.nQuads) {
            const size_t at = s.head + 4 * item;
            int32_t v[3][4];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (s.vecMask >> k & 1u) {
                    const ImgQuad<P> q = *reinterpret_cast<const ImgQuad<P> *>(planes.p[k] + at);
#pragma unroll
                    for (int i = 0; i < 4; i++) v[k][i] = (int32_t)q.v[i];
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) v[k][i] = (int32_t)planes.p[k][at + i];
                }
            }
            ImgWords x;
#pragma unroll
            for (int i = 0; i < 4; i++) x.w[i] = gf_img_join(MODEL, v[0][i], v[1][i], v[2][i]);
            *reinterpret_cast<ImgWords *>(argb + at) = x;
        } else {
            const size_t at = imgSingle(s, item);
            argb[at] = gf_img_join(MODEL, (int32_t)planes.p[0][at], (int32_t)planes.p[1][at], (int32_t)planes.p[2][at]);
        }
    }
}

// head, quads and tail of n pixels whose words start at argb, and the planes whose vectors line up with the quads
template <typename P>
ImgSpan imgSpan(const GfImageArgs &a)
{
    ImgSpan s{};
    const size_t toLine = ((16 - ((uintptr_t)a.argb & 15u)) & 15u) / 4;
    s.head = toLine < a.nPixels ? toLine : a.nPixels;
    s.nQuads = (a.nPixels - s.head) / 4;
    s.tail = a.nPixels - s.head - 4 * s.nQuads;
    for (int k = 0; k < 3; k++)
        if (((uintptr_t)a.planes[k] + s.head * sizeof(P)) % (4 * sizeof(P)) == 0) s.vecMask |= 1u << k;
    return s;
}

dim3 imgGrid(const ImgSpan &s)
{
    const size_t groups = (s.nQuads + s.head + s.tail + IMG_THREADS - 1) / IMG_THREADS;
    return dim3((uint32_t)(groups < IMG_MAX_GROUPS ? groups : IMG_MAX_GROUPS));
}

template <typename P, int MODEL>
hipError_t imgSplit(const GfImageArgs &a, hipStream_t stream)
{
    const ImgSpan s = imgSpan<P>(a);
    ImgPlanes<P> pl;
    for (int k = 0; k < 3; k++) pl.p[k] = (P *)a.planes[k];
    hipLaunchKernelGGL((k_image_split<P, MODEL>), imgGrid(s), dim3(IMG_THREADS), 0, stream, (const uint32_t *)a.argb, pl, s);
    return hipGetLastError();
}

template <typename P, int MODEL>
hipError_t imgJoin(const GfImageArgs &a, hipStream_t stream)
{
    const ImgSpan s = imgSpan<P>(a);
    ImgPlanes<const P> pl;
    for (int k = 0; k < 3; k++) pl.p[k] = (const P *)a.planes[k];
    hipLaunchKernelGGL((k_image_join<P, MODEL>), imgGrid(s), dim3(IMG_THREADS), 0, stream, pl, (uint32_t *)a.argb, s);
    return hipGetLastError();
}

bool imgArgsOk(const GfImageArgs &a)
{
    if (!a.argb || !a.planes[0] || !a.planes[1] || !a.planes[2] || a.nPixels == 0) return false;
    if (a.model != GF_IMAGE_MODEL_RGB && a.model != GF_IMAGE_MODEL_YCOCG) return false;
    return a.elemType == 0 || a.elemType == 1;
}

}  // namespace

hipError_t gf_launch_image_split(const GfImageArgs &a, hipStream_t stream)
{
    if (!imgArgsOk(a)) return hipErrorInvalidValue;
    if (a.elemType == 0) return a.model == GF_IMAGE_MODEL_RGB ? imgSplit<int32_t, GF_IMAGE_MODEL_RGB>(a, stream) : imgSplit<int32_t, GF_IMAGE_MODEL_YCOCG>(a, stream);
    return a.model == GF_IMAGE_MODEL_RGB ? imgSplit<int16_t, GF_IMAGE_MODEL_RGB>(a, stream) : imgSplit<int16_t, GF_IMAGE_MODEL_YCOCG>(a, stream);
}

hipError_t gf_launch_image_join(const GfImageArgs &a, hipStream_t stream)
{
    if (!imgArgsOk(a)) return hipErrorInvalidValue;
    if (a.elemType == 0) return a.model == GF_IMAGE_MODEL_RGB ? imgJoin<int32_t, GF_IMAGE_MODEL_RGB>(a, stream) : imgJoin<int32_t, GF_IMAGE_MODEL_YCOCG>(a, stream);
    return a.model == GF_IMAGE_MODEL_RGB ? imgJoin<int16_t, GF_IMAGE_MODEL_RGB>(a, stream) : imgJoin<int16_t, GF_IMAGE_MODEL_YCOCG>(a, stream);
}
