// gvrs_records.hip -- tile records and mixed-codec packings that already lie in device memory, in the order in which
// gvrs_api_records_dev.hip launches them: the framing walk over a record's elements (k_record_parse_elems), the records'
// CRC-32C (k_record_crc32c_elems), the partition of all element instances by codec (k_codec_partition) and, behind the codecs'
// own decode kernels, which run untouched, the pass that moves and converts decoded tiles to their place (k_elem_scatter).
// A tile holds any number of TileElementInt / Short / Float / IntCodedFloat elements (RasterTile.java:234-256 loops over
// tile.elements; TileElement*.decode); the per-element arrays are element-major (gvrs_kernels.h).
//
// Reference paths are relative to core/src/main/java/org/gridfour/: gvrs/RecordManager.java:456-459, 472-520 (readTile),
// gvrs/RasterTile.java:243-253, gvrs/CodecMaster.java:195-203, gvrs/TileElementShort.java:239-246, util/GridfourCRC32C.java.

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_crc32c.h"

namespace {

// little-endian int32 at any byte address
__device__ __forceinline__ uint32_t rec_le32(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// the class of a packing of n bytes that begins with the byte `first`: the index of its codec when the list has a decoder for the
// element's type there, else GF_REC_FAILED (empty, outside the list, or an entry without such a decoder: GF_K_ERR_FORMAT)
__device__ __forceinline__ int32_t rec_packing_class(const GfRecordParseElemsArgs &a, bool isFloat, uint32_t n, uint32_t first)
{
    if (n == 0u || (int)first >= a.nCodecs) return GF_REC_FAILED;
    // (the list's decoders for this element type as a bit set in four words: no indexed kernel argument)
    const uint64_t w = first < 64u    ? (isFloat ? a.floatSet0 : a.intSet0)
                       : first < 128u ? (isFloat ? a.floatSet1 : a.intSet1)
                       : first < 192u ? (isFloat ? a.floatSet2 : a.intSet2)
                                      : (isFloat ? a.floatSet3 : a.intSet3);
    return ((w >> (first & 63u)) & 1ull) ? (int32_t)first : GF_REC_FAILED;
}

// ------------------------------------------------------------------------------------------------
// k_record_parse_elems: a lane per record.  Record mode (a.lengths == nullptr): record t is blob[offsets[t] .. offsets[t + 1]), or
// blob[offsets[t] .. ends[t]) where a list of ends is given (records that lie anywhere in a file image, gvrs_api_file.hip); the
// framing rules of gf_tile_record_decode_batch in its order.  A record's first 20 bytes (the 16-byte head and the first byte of
// element 0, which names the codec of a packing) are fetched in one go -- every record that reaches them spans 20 bytes -- so
// that the checks behind them wait for memory once; a head that fails gives every element that status.  Then the short serial
// walk over the elements' length words: element 0's at byte 12, each next one directly behind the bytes of the one before, at any
// byte address.  An element whose length word or bytes do not fit the record is GF_K_ERR_BOUNDS, and so is every element behind it
// (they cannot be located); the ones in front keep their own class.  A packing of an INT, SHORT or ICF element must name an
// integer codec of the list, a packing of a FLOAT element an entry that is GF_CODEC_NONE (the slot of CodecFloat).
// Per instance: where its element bytes start, how many they are, its class -- failed, the standard form, or the index of its
// codec -- and the status (GF_K_OK for a packing until its decoder has spoken).  sizes[t] != 0 marks the records whose checksum the
// host call would look at: the head passed and element 0 fits (gf_tile_record_decode_batch's order).
// Packing mode (a.lengths != nullptr, one INT element): packing t is lengths[t] bytes at offsets[t] -- no head, no standard form,
// no tile index, sizes[t] = 0.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_record_parse_elems(const GfRecordParseElemsArgs a)
{
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= a.nTiles) return;
    const uint8_t *__restrict__ blob = a.blob;
    if (a.lengths) {
        const uint64_t start = a.offsets[t];
        const uint32_t n = a.lengths[t];
        int32_t st = GF_K_OK, cls = GF_REC_FAILED;
        if (start > a.blobBytes || (uint64_t)n > a.blobBytes - start) st = GF_K_ERR_BOUNDS;
        else {
            cls = rec_packing_class(a, false, n, n ? blob[start] : 0u);
            if (cls == GF_REC_FAILED) st = GF_K_ERR_FORMAT;
        }
        a.starts[t] = start;
        a.lens[t] = n;
        a.cls[t] = cls;
        a.status[t] = st;
        a.sizes[t] = 0u;
        return;
    }
    const uint64_t o0 = a.offsets[t], o1 = a.ends ? a.ends[t] : a.offsets[t + 1];
    int32_t headSt = GF_K_OK;
    uint32_t size = 0, h3 = 0, h4 = 0;
    if (o0 > o1 || o1 > a.blobBytes || o1 - o0 < 20u) headSt = GF_K_ERR_BOUNDS;          // (nothing of such a record is read)
    else {
        const uint8_t *r = blob + o0;
        uint32_t h0, h1, h2;
        if ((o0 & 3u) == 0u) {
            const GfU4 q = *reinterpret_cast<const GfU4 *>(r);
            h4 = *reinterpret_cast<const uint32_t *>(r + 16);
            h0 = q.x, h1 = q.y, h2 = q.z, h3 = q.w;
        } else {
            h0 = rec_le32(r), h1 = rec_le32(r + 4), h2 = rec_le32(r + 8), h3 = rec_le32(r + 12), h4 = r[16];
        }
        size = h0;
        if ((uint64_t)size > o1 - o0 || size < 20u || (size & 7u)) headSt = GF_K_ERR_BOUNDS;
        else if ((h1 & 0xffu) != 2u) headSt = GF_K_ERR_FORMAT;                            // not RecordType.Tile
        else if (a.tileIndices) a.tileIndices[t] = (int32_t)h2;
    }
    const uint8_t *r = blob + o0;
    bool located = headSt == GF_K_OK;                       // the next element's length word is known to be at r + pos
    uint32_t pos = 12, crcSize = 0;
    for (int e = 0; e < a.nElems; e++) {
        int32_t st = headSt, cls = GF_REC_FAILED;
        uint64_t start = 0;
        uint32_t n = 0;
        if (headSt == GF_K_OK) {
            st = GF_K_ERR_BOUNDS;
            if (located && (uint64_t)pos + 4u <= size) n = e == 0 ? h3 : rec_le32(r + pos);
            else located = false;
            if (located && (uint64_t)pos + 4u + n > size) located = false;
            if (located) {
                const uint32_t type = (a.elemTypes >> (2 * e)) & 3u;
                // TileElement.java:86-93: bytes per sample * cells, rounded up to a multiple of 4
                const uint32_t stdSize = type == (uint32_t)GF_K_ELEM_SHORT ? ((a.cells * 2u + 3u) & ~3u) : a.cells * 4u;
                start = o0 + pos + 4u;
                st = GF_K_OK;
                if (e == 0) crcSize = size;
                if (n == stdSize) cls = GF_REC_STANDARD;
                else {
                    const uint32_t first = n == 0u ? 0u : e == 0 ? (h4 & 0xffu) : (uint32_t)r[pos + 4u];
                    cls = rec_packing_class(a, type == (uint32_t)GF_K_ELEM_FLOAT, n, first);
                    if (cls == GF_REC_FAILED) st = GF_K_ERR_FORMAT;
                }
                pos += 4u + n;
            }
        }
        const size_t i = (size_t)e * a.nTiles + t;
        a.starts[i] = start;
        a.lens[i] = n;
        a.cls[i] = cls;
        a.status[i] = st;
    }
    a.sizes[t] = crcSize;
}

// ------------------------------------------------------------------------------------------------
// k_record_crc32c_elems: verification only.  A wave per record with sizes[t] != 0: the CRC-32C of its first size - 4 bytes against
// the stored one in its last four (wave_crc_bytes, gvrs_crc32c.h).  A record that starts at a multiple of 4 (file records start at
// multiples of 8) is read in 16-byte and 4-byte pieces, any other byte by byte.  Nothing outside [offsets[t], offsets[t] + size) is read.
// A mismatch reaches all nElems instances of the record (lane e writes element e's): class failed -- out of the partition --
// and GF_K_ERR_FORMAT, whatever the walk said about them.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_record_crc32c_elems(const uint8_t *__restrict__ blob, const uint64_t *__restrict__ offsets,
                                                             const uint32_t *__restrict__ sizes, int32_t *__restrict__ cls,
                                                             int32_t *__restrict__ status, size_t nTiles, int nElems)
{
    __shared__ uint32_t table[256];
    crc_table_fill_256(table);
    const uint32_t lane = threadIdx.x & 63u;
    const size_t t = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (t >= nTiles) return;
    const uint32_t size = sizes[t];
    if (size == 0u) return;
    const uint64_t o0 = offsets[t];
    const uint32_t nBytes = size - 4u;
    const uint8_t *__restrict__ r = blob + o0;
    const uint32_t part = wave_crc_bytes(table, r, nBytes, lane, (o0 & 3u) == 0u, true);
    if ((int)lane < nElems && part != rec_le32(r + nBytes)) {
        status[(size_t)lane * nTiles + t] = GF_K_ERR_FORMAT;
        cls[(size_t)lane * nTiles + t] = GF_REC_FAILED;
    }
}

// ------------------------------------------------------------------------------------------------
// k_codec_partition: ONE workgroup sorts the batch's records by class, stably: segment s < nCodecs holds the packings of codec s in
// record order, segment nCodecs the records in standard form; the segments follow one another in the three output arrays
// (subOffsets: where the element bytes start in the blob, subLengths, subDst: the record's number) and counts[s] says how long each
// is.  First the segment totals (LDS counters), then 1,024 records at a time: a wave finds each member's rank among its own lanes
// with one ballot per segment present in the wave, the waves' counts meet in LDS, and a record's place is its segment's start + the
// members before this round + those in earlier waves + its rank.  No global atomics; the order never depends on timing.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t PART_THREADS = 1024, PART_WAVES = PART_THREADS / 64, PART_SEGS = 256;

__global__ __launch_bounds__(PART_THREADS) void k_codec_partition(const GfPartitionArgs a)
{
    __shared__ uint32_t waveCnt[PART_WAVES][PART_SEGS];
    __shared__ uint32_t segBase[PART_SEGS], run[PART_SEGS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nSeg = (uint32_t)a.nCodecs + 1u;
    if (tid < PART_SEGS) run[tid] = 0u;
    for (uint32_t i = tid; i < PART_WAVES * PART_SEGS; i += PART_THREADS) (&waveCnt[0][0])[i] = 0u;
    __syncthreads();
    for (size_t t = tid; t < a.nTiles; t += PART_THREADS) {
        const int32_t c = a.cls[t];
        if (c != GF_REC_FAILED) atomicAdd(&run[c == GF_REC_STANDARD ? nSeg - 1u : (uint32_t)c], 1u);     // (LDS)
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t base = 0;
        for (uint32_t s = 0; s < nSeg; s++) {
            segBase[s] = base;
            base += run[s];
        }
    }
    __syncthreads();
    if (tid < nSeg) {
        a.counts[tid] = run[tid];
        run[tid] = 0u;
    }
    __syncthreads();
    for (size_t t0 = 0; t0 < a.nTiles; t0 += PART_THREADS) {
        const size_t t = t0 + tid;
        int32_t seg = -1;
        if (t < a.nTiles) {
            const int32_t c = a.cls[t];
            seg = c == GF_REC_FAILED ? -1 : c == GF_REC_STANDARD ? (int32_t)nSeg - 1 : c;
        }
        uint32_t rank = 0;
        uint64_t todo = __ballot(seg >= 0);
        while (todo) {                                                         // (wave-uniform)
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const int32_t s = __shfl(seg, leader);
            const uint64_t m = __ballot(seg == s);
            if (seg == s) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if ((int)lane == leader) waveCnt[wave][s] = (uint32_t)__popcll(m);
            todo &= ~m;
        }
        __syncthreads();
        if (seg >= 0) {
            uint32_t before = 0;
            for (uint32_t w = 0; w < wave; w++) before += waveCnt[w][seg];
            const uint32_t j = segBase[seg] + run[seg] + before + rank;
            a.subOffsets[j] = a.starts[t];
            a.subLengths[j] = a.lens[t];
            a.subDst[j] = (uint32_t)t;
        }
        __syncthreads();
        if (tid < nSeg) {
            uint32_t sum = 0;
            for (uint32_t w = 0; w < PART_WAVES; w++) {
                sum += waveCnt[w][tid];
                waveCnt[w][tid] = 0u;
            }
            run[tid] += sum;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// k_elem_scatter: a workgroup per entry of the partition; the entry's instance number says which element of which record it is.
// Decoded tiles (entries below nPacked) go from the temporary to their place when their decoder said GF_K_OK: INT and FLOAT cells
// copied, SHORT narrowed (INT4_NULL_CODE -> -32768), ICF converted; the decoder's status to status[instance].  The entries behind
// them are elements in standard form: INT, FLOAT and SHORT cells copied from wherever they lie in the blob, ICF converted from
// raw little-endian ints at any byte alignment.  Every path issues its loads before its stores and leaves the wave in rows of
// 16 (8, 4, 2) bytes per lane (DESIGN section 8 on requests and on loads queued behind stores).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rec_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, size_t nBytes)
{
    const uintptr_t both = (uintptr_t)dst | (uintptr_t)src | (uintptr_t)nBytes;
    if ((both & 15u) == 0u) {
        for (size_t i = (size_t)threadIdx.x * 16u; i < nBytes; i += (size_t)blockDim.x * 16u)
            *reinterpret_cast<uint4 *>(dst + i) = *reinterpret_cast<const uint4 *>(src + i);
    } else if ((both & 7u) == 0u) {
        for (size_t i = (size_t)threadIdx.x * 8u; i < nBytes; i += (size_t)blockDim.x * 8u)
            *reinterpret_cast<uint2 *>(dst + i) = *reinterpret_cast<const uint2 *>(src + i);
    } else if ((both & 3u) == 0u) {
        for (size_t i = (size_t)threadIdx.x * 4u; i < nBytes; i += (size_t)blockDim.x * 4u)
            *reinterpret_cast<uint32_t *>(dst + i) = *reinterpret_cast<const uint32_t *>(src + i);
    } else {
        for (size_t i = threadIdx.x; i < nBytes; i += blockDim.x) dst[i] = src[i];
    }
}

__device__ __forceinline__ uint32_t rec_narrow2(uint32_t lo, uint32_t hi)     // two cells -> two shorts in a word
{
    lo = lo == GF_NULL_CODE ? 0x8000u : (lo & 0xffffu);
    hi = hi == GF_NULL_CODE ? 0x8000u : (hi & 0xffffu);
    return lo | (hi << 16);
}

// TileElementIntCodedFloat.java:172-176: values[index] / scale + offset in single precision, each step rounded once
__device__ __forceinline__ uint32_t rec_icf(uint32_t code, const GfElemDesc &d)
{
    const float v = __fadd_rn(__fdiv_rn((float)(int32_t)code, d.scale), d.offset);
    return (int32_t)code == d.fillI ? __float_as_uint(d.fillF) : __float_as_uint(v);
}

__device__ __forceinline__ uint4 rec_icf4(const uint4 c, const GfElemDesc &d)
{
    uint4 o;
    o.x = rec_icf(c.x, d), o.y = rec_icf(c.y, d), o.z = rec_icf(c.z, d), o.w = rec_icf(c.w, d);
    return o;
}

// cells ints at src (any byte address) -> floats at dst: eight cells per lane, then four, in 16-byte pieces where both sides are
// 16-byte aligned, and a tail of single cells; single words where only the source is 4-byte aligned; bytes otherwise
__device__ __forceinline__ void rec_icf_tile(uint32_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t cells, const GfElemDesc &d)
{
    if ((((uintptr_t)dst | (uintptr_t)src) & 15u) == 0u) {
        const uint32_t n8 = cells & ~7u, n4 = cells & ~3u;
#pragma unroll 1
        for (uint32_t i = threadIdx.x * 8u; i < n8; i += 256u * 8u) {
            const uint4 p = *reinterpret_cast<const uint4 *>(src + (size_t)i * 4u), q = *reinterpret_cast<const uint4 *>(src + (size_t)i * 4u + 16u);
            const uint4 u = rec_icf4(p, d), v = rec_icf4(q, d);
            *reinterpret_cast<uint4 *>(dst + i) = u;
            *reinterpret_cast<uint4 *>(dst + i + 4) = v;
        }
        if (threadIdx.x == 0 && n4 > n8) *reinterpret_cast<uint4 *>(dst + n8) = rec_icf4(*reinterpret_cast<const uint4 *>(src + (size_t)n8 * 4u), d);
        if (n4 + threadIdx.x < cells) dst[n4 + threadIdx.x] = rec_icf(*reinterpret_cast<const uint32_t *>(src + (size_t)(n4 + threadIdx.x) * 4u), d);
    } else if (((uintptr_t)src & 3u) == 0u) {
#pragma unroll 1
        for (uint32_t i = threadIdx.x; i < cells; i += 256u) dst[i] = rec_icf(*reinterpret_cast<const uint32_t *>(src + (size_t)i * 4u), d);
    } else {
#pragma unroll 1
        for (uint32_t i = threadIdx.x; i < cells; i += 256u) dst[i] = rec_icf(rec_le32(src + (size_t)i * 4u), d);
    }
}

// decoded cells -> shorts (TileElementShort.java:239-246)
__device__ __forceinline__ void rec_narrow_tile(int16_t *__restrict__ out, const int32_t *__restrict__ src, uint32_t cells)
{
    if ((cells & 7u) == 0u && (((uintptr_t)out | (uintptr_t)src) & 15u) == 0u) {
        for (uint32_t i = threadIdx.x * 8u; i < cells; i += 256u * 8u) {
            const uint4 p = *reinterpret_cast<const uint4 *>(src + i), q = *reinterpret_cast<const uint4 *>(src + i + 4);
            uint4 o;
            o.x = rec_narrow2(p.x, p.y), o.y = rec_narrow2(p.z, p.w), o.z = rec_narrow2(q.x, q.y), o.w = rec_narrow2(q.z, q.w);
            *reinterpret_cast<uint4 *>(out + i) = o;
        }
    } else {
        for (uint32_t i = threadIdx.x; i < cells; i += 256u) {
            const int32_t v = src[i];
            out[i] = v == (int32_t)GF_NULL_CODE ? (int16_t)-32768 : (int16_t)v;
        }
    }
}

// (8 waves per SIMD asked for: left alone the compiler interleaves the eight divisions of the ICF loop over 113 VGPRs, 4 waves per SIMD for
// every path of a kernel that is bandwidth; held to 64 it needs 58 and no scratch)
__global__ __launch_bounds__(256, 8) void k_elem_scatter(const GfElemScatterArgs a)
{
    GF_FOR_WG_TILE(j, a.nTotal)
    {
        const uint32_t inst = a.subDst[j], e = inst / (uint32_t)a.nTiles;
        const size_t t = inst - (size_t)e * a.nTiles, cells = a.cells;
        const GfElemDesc d = a.elems[e];                                       // (workgroup-uniform: scalar loads)
        const uint8_t *__restrict__ src;
        if (j >= a.nPacked) src = a.blob + a.subOffsets[j];
        else {
            const int32_t st = a.subStatus[j];
            if (threadIdx.x == 0) a.status[inst] = st;
            if (st != GF_K_OK) continue;
            src = reinterpret_cast<const uint8_t *>(a.tmp + j * cells);
        }
        if (d.type == GF_K_ELEM_ICF) rec_icf_tile(reinterpret_cast<uint32_t *>(d.values) + t * cells, src, (uint32_t)cells, d);
        else if (d.type != GF_K_ELEM_SHORT) rec_copy(reinterpret_cast<uint8_t *>(d.values) + t * cells * 4u, src, cells * 4u);
        else if (j >= a.nPacked) rec_copy(reinterpret_cast<uint8_t *>(d.values) + t * cells * 2u, src, cells * 2u);
        else rec_narrow_tile(reinterpret_cast<int16_t *>(d.values) + t * cells, reinterpret_cast<const int32_t *>(src), (uint32_t)cells);
    }
}

}  // namespace

hipError_t gf_launch_record_parse_elems(const GfRecordParseElemsArgs &a, hipStream_t stream)
{
    if (a.nElems < 1 || a.nElems > GF_K_MAX_ELEMS) return hipErrorInvalidValue;
    if (a.lengths && (a.nElems != 1 || a.elemTypes != (uint32_t)GF_K_ELEM_INT)) return hipErrorInvalidValue;
    if (a.nTiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_record_parse_elems, dim3((unsigned)((a.nTiles + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_record_crc32c_elems(const uint8_t *blob, const uint64_t *offsets, const uint32_t *sizes, int32_t *cls, int32_t *status,
                                         size_t nTiles, int nElems, hipStream_t stream)
{
    if (nTiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_record_crc32c_elems, dim3((unsigned)((nTiles + 3) / 4)), dim3(256), 0, stream, blob, offsets, sizes, cls, status,
                       nTiles, nElems);
    return hipGetLastError();
}

hipError_t gf_launch_codec_partition(const GfPartitionArgs &a, hipStream_t stream)
{
    if (a.nCodecs < 0 || a.nCodecs > 255) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_codec_partition, dim3(1), dim3(PART_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_elem_scatter(const GfElemScatterArgs &a, hipStream_t stream)
{
    if (a.nTotal == 0) return hipSuccess;
    hipLaunchKernelGGL(k_elem_scatter, gf_tile_grid(a.nTotal), dim3(256), 0, stream, a);
    return hipGetLastError();
}
