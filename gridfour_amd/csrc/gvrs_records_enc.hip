// gvrs_records_enc.hip -- tile records WRITTEN in device memory, in the order in which gvrs_api_records_enc.hip launches them: the
// widening of SHORT cells for the codecs (k_elem_widen), behind the codecs' own encoders, which run untouched, the CodecMaster
// selection and the record layout (k_record_plan), the scan of the record sizes (k_record_scan), the byte-granular assembly of the
// records (k_record_write) and their CRC-32C (k_record_crc32c_write).  The mirror image of gvrs_records.hip.
//
// Reference paths are relative to core/src/main/java/org/gridfour/: gvrs/RecordManager.java:386-490 (writeTile),
// gvrs/RasterTile.java:234-256 (getCompressedPacking), gvrs/TileElementInt.java:196-206, gvrs/TileElementShort.java:100-110, 211-229,
// gvrs/TileElementFloat.java:209-219, gvrs/CodecMaster.java:150-169, 261-280, util/GridfourCRC32C.java.
//
// The whole-tile rule (RecordManager.java:417-431 stores the compressed form only if 4 + packing < payload) changes no byte and has
// no branch here: every element's n is <= its standard size, so the rule fails only when every element is already in standard form,
// and the uncompressed branch (:483-487) then writes the same [standard size][standard form] sequence per element.

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_crc32c.h"

namespace {

// ------------------------------------------------------------------------------------------------
// k_elem_widen: bandwidth.  Four cells per lane and turn: an 8-byte load, a 16-byte store; the last nCells % 4 cells one by one.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t widen1(uint32_t s, uint32_t fill)
{
    return s == fill ? GF_NULL_CODE : (uint32_t)(int32_t)(int16_t)s;
}

__global__ __launch_bounds__(256) void k_elem_widen(const int16_t *__restrict__ src, int32_t *__restrict__ dst, size_t nCells, uint32_t fill)
{
    const size_t n4 = nCells >> 2, stride = (size_t)gridDim.x * 256u;
    for (size_t q = (size_t)blockIdx.x * 256u + threadIdx.x; q < n4; q += stride) {
        const GfU2 p = *reinterpret_cast<const GfU2 *>(src + q * 4u);
        uint4 o;
        o.x = widen1(p.x & 0xffffu, fill), o.y = widen1(p.x >> 16, fill), o.z = widen1(p.y & 0xffffu, fill), o.w = widen1(p.y >> 16, fill);
        *reinterpret_cast<uint4 *>(dst + q * 4u) = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (nCells & 3u)) {
        const size_t i = n4 * 4u + threadIdx.x;
        dst[i] = (int32_t)widen1((uint16_t)src[i], fill);
    }
}

// ------------------------------------------------------------------------------------------------
// k_record_plan: a lane per tile.  Per element the CodecMaster selection over its candidates (CodecMaster.java:150-169: the strictly
// shortest non-null packing, list order on ties -- as gf_codec_master_encode_batch_i32 decides) and the per-element rule "not
// shorter than the standard form -> the standard form" (TileElementInt.java:198-204): a candidate that declined, overflowed its
// slot (the slot is at least as long as the standard form) or measures >= the standard size loses.  An encoder that failed (a
// negative status: the Java encoder would throw) fails the record: size 0, nothing of it is written; a non-zero pre-status (a block
// write's verdict: an unreadable old record, a cell out of range, no valid data) does the same and is the record's status.  The
// element descriptions are kernel arguments (scalar loads).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_record_plan(const GfRecordPlanArgs a)
{
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= a.nTiles) return;
    uint32_t pos = 12;                                                      // behind size, type and tile index
    int32_t st = GF_K_OK;
    for (int e = 0; e < a.nElems; e++) {
        const uint32_t stdSize = a.elems[e].stdSize, cand0 = a.elems[e].cand0;
        const bool hasCand = a.elems[e].slots != nullptr;
        uint32_t best = 255u, bestLen = 0u;
        if (hasCand) {
            for (int k = 0; k < a.nAct; k++) {
                const size_t c = (size_t)(cand0 + (uint32_t)k) * a.nTiles + t;
                const int32_t s = a.candStatus[c];
                const uint32_t len = a.candLen[c];
                if (s < 0) {
                    if (st == GF_K_OK) st = s;
                    continue;
                }
                if (s != GF_K_OK || len == 0u || len >= stdSize) continue;
                if (best == 255u || len < bestLen) best = (uint32_t)k, bestLen = len;
            }
        }
        const uint32_t n = best == 255u ? stdSize : bestLen;
        const size_t i = (size_t)e * a.nTiles + t;
        a.elemLen[i] = n;
        a.elemPos[i] = pos;
        a.elemSrc[i] = (uint8_t)best;
        if (a.codecUsed) a.codecUsed[i] = best == 255u ? (uint8_t)255u : a.actIndex[best];
        pos += 4u + n;
    }
    const int32_t pre = a.preStatus ? a.preStatus[t] : 0;                   // the caller's verdict comes before the encoders'
    if (pre != 0) {
        st = pre;
        if (a.codecUsed)
            for (int e = 0; e < a.nElems; e++) a.codecUsed[(size_t)e * a.nTiles + t] = (uint8_t)255u;
    }
    a.sizes[t] = st == GF_K_OK ? ((pos + 4u + 7u) & ~7u) : 0u;               // multipleOf8(4 + content + RECORD_OVERHEAD_SIZE)
    a.status[t] = st;
}

// ------------------------------------------------------------------------------------------------
// k_record_scan: ONE workgroup, 1,024 records a turn (the shape of k_scan_lengths in gvrs_aux.hip): offsets = exclusive scan of sizes
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_record_scan(const uint32_t *__restrict__ sizes, uint64_t *__restrict__ offsets, size_t nTiles)
{
    __shared__ unsigned long long waveSum[16];
    __shared__ unsigned long long carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (size_t base = 0; base < nTiles; base += 1024) {
        const size_t i = base + tid;
        const unsigned long long v = i < nTiles ? sizes[i] : 0ull;
        unsigned long long incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) waveSum[wave] = incl;
        __syncthreads();
        unsigned long long pre = carry, tot = 0;
        for (int w = 0; w < 16; w++) {
            if (w < wave) pre += waveSum[w];
            tot += waveSum[w];
        }
        if (i < nTiles) offsets[i] = pre + incl - v;
        __syncthreads();
        if (tid == 0) carry += tot;
        __syncthreads();
    }
    if (tid == 0) offsets[nTiles] = carry;
}

// ------------------------------------------------------------------------------------------------
// k_record_write: a workgroup per element and record (a record of sixteen small elements is sixteen workgroups' work, not one
// serial loop, and each workgroup's share is one contiguous piece of the record): element e's workgroup writes its length word and
// its n bytes; element 0's also the record's first twelve bytes, the last element's the zero padding and, without checksums, the
// zero checksum word.  Every byte of a written record is stored exactly once.
// The element's bytes start at ANY byte of the record and come from a 16-byte aligned slot, a 4-byte aligned int32 / float tile or
// a 2-byte aligned int16 tile.  The body moves as 16-byte stores aligned on the destination; a lane loads the 16 (or, where
// source and destination disagree modulo 4, 20) bytes it needs as a 16-byte load and a word at 4-byte aligned addresses and
// shifts them into place (v_alignbyte), two pieces a turn, loads before stores; a wave's stores are consecutive pieces of one
// record.  Only the edges (up to 15 bytes in front, up to 15 + 16 behind -- the piece that holds the two zero bytes of an odd
// SHORT tile) go byte by byte.  Nothing is read outside the packing or the tile's cells rounded out to aligned words.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 rec_load16(const uint8_t *__restrict__ s)
{
    const uint32_t sh = (uint32_t)((uintptr_t)s & 3u);
    const uint8_t *base = s - sh;
    const GfU4 w = *reinterpret_cast<const GfU4 *>(base);
    uint4 o;
    if (sh == 0u) {
        o.x = w.x, o.y = w.y, o.z = w.z, o.w = w.w;
    } else {
        const uint32_t x = *reinterpret_cast<const uint32_t *>(base + 16);   // (holds byte s + 16 - sh .. : at least one byte of the piece)
        o.x = __builtin_amdgcn_alignbyte(w.y, w.x, sh);
        o.y = __builtin_amdgcn_alignbyte(w.z, w.y, sh);
        o.z = __builtin_amdgcn_alignbyte(w.w, w.z, sh);
        o.w = __builtin_amdgcn_alignbyte(x, w.w, sh);
    }
    return o;
}

__global__ __launch_bounds__(256) void k_record_write(const GfRecordWriteArgs a)
{
    GF_FOR_WG_TILE(j, a.nTiles * (size_t)a.nElems)
    {
        const size_t t = j / (size_t)a.nElems;
        const int e = (int)(j - t * (size_t)a.nElems);
        const uint32_t size = a.sizes[t];
        if (size == 0u) continue;                                           // an encoder failed: the record has no bytes
        const uint64_t o0 = a.offsets[t];
        if (o0 + size > a.blobCap) continue;                                // skipped whole; offsets[nTiles] > blobCap tells the caller
        uint8_t *__restrict__ r = a.blob + o0;
        const uint32_t tid = threadIdx.x;
        const size_t i = (size_t)e * a.nTiles + t;
        const uint32_t n = a.elemLen[i], pos = a.elemPos[i], sel = a.elemSrc[i];
        const uint32_t stdBytes = a.elems[e].srcBytes, stride = a.elems[e].slotStride;
        const uint8_t *__restrict__ src;
        uint32_t nSrc;
        if (sel == 255u) {
            src = reinterpret_cast<const uint8_t *>(a.elems[e].values) + t * (size_t)stdBytes;
            nSrc = stdBytes;                                                // (n - nSrc = 0 or 2: the zero short of an odd SHORT tile)
        } else {
            src = a.elems[e].slots + ((size_t)sel * a.nTiles + t) * (size_t)stride;
            nSrc = n;
        }
        if (e == 0 && tid < 3u)                                             // [size][type 2, 0 0 0][tile index]: the record is 8-byte aligned
            reinterpret_cast<uint32_t *>(r)[tid] = tid == 0u ? size : tid == 1u ? 2u : (uint32_t)a.tileIndices[t];
        if (tid >= 64u && tid < 68u) r[pos + (tid - 64u)] = (uint8_t)(n >> (8u * (tid - 64u)));
        uint8_t *__restrict__ dst = r + pos + 4u;
        const uint32_t head = min(n, (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
        const uint32_t nq = nSrc > head ? (nSrc - head) >> 4 : 0u;          // 16-byte pieces of the destination that the source fills
#pragma unroll 1
        for (uint32_t q = tid; q < nq; q += 512u) {
            const uint32_t b0 = head + 16u * q, q1 = q + 256u;
            const uint4 p0 = rec_load16(src + b0);
            if (q1 < nq) {
                const uint32_t b1 = head + 16u * q1;
                const uint4 p1 = rec_load16(src + b1);
                *reinterpret_cast<uint4 *>(dst + b0) = p0;
                *reinterpret_cast<uint4 *>(dst + b1) = p1;
            } else {
                *reinterpret_cast<uint4 *>(dst + b0) = p0;
            }
        }
        // the edges: [0, head) and [head + 16 nq, n), fewer than 64 bytes together
        {
            const uint32_t b = tid < head ? tid : head + 16u * nq + (tid - head);
            if (tid < 64u && b < n) dst[b] = b < nSrc ? src[b] : (uint8_t)0;
        }
        if (e == a.nElems - 1) {                                            // zeros up to the checksum word, or through it
            const uint32_t z0 = pos + 4u + n, z1 = a.checksum ? size - 4u : size;
            if (tid >= 128u && z0 + (tid - 128u) < z1) r[z0 + (tid - 128u)] = 0;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_record_crc32c_write: a wave per written record, as k_record_crc32c_elems reads one (wave_crc_bytes, gvrs_crc32c.h), and lane 0
// stores the checksum into the record's last word (a vector store).  Records start at multiples of 8: 16-byte and 4-byte loads
// throughout.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_record_crc32c_write(uint8_t *__restrict__ blob, size_t blobCap, const uint64_t *__restrict__ offsets,
                                                             const uint32_t *__restrict__ sizes, size_t nTiles)
{
    __shared__ uint32_t table[256];
    crc_table_fill_256(table);
    const uint32_t lane = threadIdx.x & 63u;
    const size_t t = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (t >= nTiles) return;
    const uint32_t size = sizes[t];
    if (size == 0u) return;
    const uint64_t o0 = offsets[t];
    if (o0 + size > blobCap) return;
    const uint32_t nBytes = size - 4u;                                        // (a multiple of 4)
    uint8_t *r = blob + o0;
    const uint32_t part = wave_crc_bytes(table, r, nBytes, lane, true, false);
    if (lane == 0u) *reinterpret_cast<uint32_t *>(r + nBytes) = part;
}

}  // namespace

hipError_t gf_launch_elem_widen(const int16_t *src, int32_t *dst, size_t nCells, int fill, hipStream_t stream)
{
    if (nCells == 0) return hipSuccess;
    const size_t groups = (nCells / 4 + 255) / 256;
    const unsigned grid = (unsigned)(groups < 1 ? 1 : groups > 16384 ? 16384 : groups);
    hipLaunchKernelGGL(k_elem_widen, dim3(grid), dim3(256), 0, stream, src, dst, nCells, (uint32_t)(uint16_t)(int16_t)fill);
    return hipGetLastError();
}

hipError_t gf_launch_record_plan(const GfRecordPlanArgs &a, hipStream_t stream)
{
    if (a.nElems < 1 || a.nElems > GF_K_MAX_ELEMS || a.nAct < 0 || a.nAct > 255) return hipErrorInvalidValue;
    if (a.nTiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_record_plan, dim3((unsigned)((a.nTiles + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_record_scan(const uint32_t *sizes, uint64_t *offsets, size_t nTiles, hipStream_t stream)
{
    hipLaunchKernelGGL(k_record_scan, dim3(1), dim3(1024), 0, stream, sizes, offsets, nTiles);
    return hipGetLastError();
}

hipError_t gf_launch_record_write(const GfRecordWriteArgs &a, hipStream_t stream)
{
    if (a.nElems < 1 || a.nElems > GF_K_MAX_ELEMS || ((uintptr_t)a.blob & 7u) != 0) return hipErrorInvalidValue;
    if (a.nTiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_record_write, gf_tile_grid(a.nTiles * (size_t)a.nElems), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_record_crc32c_write(uint8_t *blob, size_t blobCap, const uint64_t *offsets, const uint32_t *sizes, size_t nTiles,
                                         hipStream_t stream)
{
    if (nTiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_record_crc32c_write, dim3((unsigned)((nTiles + 3) / 4)), dim3(256), 0, stream, blob, blobCap, offsets, sizes, nTiles);
    return hipGetLastError();
}
