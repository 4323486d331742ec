// gvrs_aux.hip -- small helper kernels: packing compaction and the synthetic DEM generator; and the two kernels of
// CodecCanonHuffman.analyze (k_canon_decode<true>, k_canon_stats), kept out of gvrs_canon_decode.hip's translation unit
// (see gvrs_canon_decode_kernel.h).

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "huff_build.h"

namespace {

// ---- compaction: exclusive scan of the lengths (one workgroup), then one workgroup per tile copies ----
// status (optional): a tile whose status is not GF_K_OK contributes no bytes; nor does a tile whose length is greater than the
// slot stride (an encoder reported GF_OVERFLOW, "length is still reported", and left the slot untouched: there is nothing to copy,
// and len bytes from the slot's start would run through the following slots and past the end of the slot array)
__device__ __forceinline__ uint32_t compact_len(const uint32_t *__restrict__ lengths, const int32_t *__restrict__ status, size_t t,
                                                size_t slotStride)
{
    if (status && status[t] != GF_K_OK) return 0u;
    const uint32_t len = lengths[t];
    return len > slotStride ? 0u : len;
}

__global__ __launch_bounds__(1024) void k_scan_lengths(size_t nTiles, size_t slotStride, const uint32_t *__restrict__ lengths,
                                                       const int32_t *__restrict__ status, uint64_t *__restrict__ offsets)
{
    __shared__ unsigned long long waveSum[16];
    __shared__ unsigned long long carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (size_t base = 0; base < nTiles; base += 1024) {
        const size_t i = base + tid;
        const unsigned long long v = i < nTiles ? compact_len(lengths, status, i, slotStride) : 0ull;
        unsigned long long incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            unsigned long long t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
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

__global__ __launch_bounds__(256) void k_gather(size_t nTiles, const uint8_t *__restrict__ slots, size_t slotStride,
                                                const uint32_t *__restrict__ lengths, const int32_t *__restrict__ status,
                                                const uint64_t *__restrict__ offsets, uint8_t *__restrict__ blob,
                                                size_t blobCap)
{
    for (size_t t = blockIdx.x; t < nTiles; t += gridDim.x) {
        const uint8_t *src = slots + t * slotStride;
        const uint64_t off = offsets[t];
        const uint32_t len = compact_len(lengths, status, t, slotStride);
        if (off + len > blobCap) continue;
        uint8_t *dst = blob + off;
        // head bytes up to 4-byte alignment of dst, then dwords assembled from the (aligned) slot
        const uint32_t mis = (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3);
        const uint32_t head = mis < len ? mis : len;
        for (uint32_t i = threadIdx.x; i < head; i += blockDim.x) dst[i] = src[i];
        const uint32_t nw = (len - head) >> 2;
        const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src);   // slots are 16-byte aligned
        uint32_t *d32 = reinterpret_cast<uint32_t *>(dst + head);
        for (uint32_t w = threadIdx.x; w < nw; w += blockDim.x) {
            const uint32_t b = head + 4 * w;                             // source byte offset
            // the word behind lo only where it still holds bytes of the packing (never read behind the slot)
            const uint32_t lo = s32[b >> 2], hi = ((b >> 2) + 1u < ((len + 3u) >> 2)) ? s32[(b >> 2) + 1] : 0u;
            const uint32_t sh = (b & 3) * 8;
            d32[w] = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
        }
        for (uint32_t i = head + 4 * nw + threadIdx.x; i < len; i += blockDim.x) dst[i] = src[i];
    }
}

// ---- synthetic DEM: integer value noise, same integer recipe as the test-side CPU generator ----
__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__device__ __forceinline__ int32_t dem_lattice(uint64_t seed, int o, int64_t i, int64_t j)
{
    const uint64_t h = splitmix64(seed ^ ((uint64_t)o << 56) ^ (((uint64_t)j & 0xFFFFFFFULL) << 28) ^
                                  ((uint64_t)i & 0xFFFFFFFULL));
    const int32_t amp = 4096 >> o;
    return (int32_t)((((h >> 32) & 0xFFFF) * (uint64_t)(2 * amp)) >> 16) - amp;
}

__device__ int32_t dem_value(uint64_t seed, int64_t gx, int64_t gy)
{
    int64_t sum = 0;
    for (int o = 0; o < 6; o++) {
        const int sh = 8 - o;
        const int64_t s = (int64_t)1 << sh;
        const int64_t i = gx >> sh, j = gy >> sh;
        const int64_t fx = gx & (s - 1), fy = gy & (s - 1);
        const int64_t l00 = dem_lattice(seed, o, i, j), l10 = dem_lattice(seed, o, i + 1, j);
        const int64_t l01 = dem_lattice(seed, o, i, j + 1), l11 = dem_lattice(seed, o, i + 1, j + 1);
        const int64_t top = l00 * (s - fx) + l10 * fx;
        const int64_t bot = l01 * (s - fx) + l11 * fx;
        sum += (top * (s - fy) + bot * fy) >> (2 * sh);
    }
    const uint64_t h = splitmix64(seed ^ 0x7700000000000000ULL ^ (((uint64_t)gy & 0xFFFFFFFULL) << 28) ^
                                  ((uint64_t)gx & 0xFFFFFFFULL));
    sum += (int64_t)((h >> 40) % 5) - 2;
    sum -= 2000;
    if (sum < -11000) sum = -11000;
    if (sum > 8848) sum = 8848;
    return (int32_t)sum;
}

// The rough surface (style 1, round 4; SURVEY.md 8d asks for "a tail into 2-3 byte codes", which the classic surface does not
// have): provinces of 1024 x 1024 cells -- mountains (the classic surface), plains (a sixteenth of the largest octave's relief
// under jitter of -6..6: PredictorModelDifferencing wins), stripes (every row samples the classic surface 37 rows further on:
// PredictorModelLinear wins) -- and, on hashed 16 x 16 blocks, cliffs (one more octave: lattice spacing 4, amplitude 520) and
// scree (white noise of -150..150): row differences that need two and three M32 bytes (CodecM32.java:270-311).  Same integer
// recipe as the test-side generator; the statistics are in its comment and in the bench line.
constexpr int DEM_PROVINCE_SHIFT = 10;
constexpr int64_t DEM_CLIFF_AMP = 520;
constexpr uint32_t DEM_SCREE_AMP = 150;
__device__ __forceinline__ int64_t dem_octaves(uint64_t seed, int64_t gx, int64_t gy, int first, int last)
{
    int64_t sum = 0;
    for (int o = first; o < last; o++) {
        const int sh = 8 - o;
        const int64_t s = (int64_t)1 << sh;
        const int64_t i = gx >> sh, j = gy >> sh;
        const int64_t fx = gx & (s - 1), fy = gy & (s - 1);
        const int64_t l00 = dem_lattice(seed, o, i, j), l10 = dem_lattice(seed, o, i + 1, j);
        const int64_t l01 = dem_lattice(seed, o, i, j + 1), l11 = dem_lattice(seed, o, i + 1, j + 1);
        const int64_t top = l00 * (s - fx) + l10 * fx;
        const int64_t bot = l01 * (s - fx) + l11 * fx;
        sum += (top * (s - fy) + bot * fy) >> (2 * sh);
    }
    return sum;
}
__device__ int32_t dem_value_rough(uint64_t seed, int64_t gx, int64_t gy)
{
    const uint64_t hp = splitmix64(seed ^ 0x5500000000000000ULL ^ ((((uint64_t)gy >> DEM_PROVINCE_SHIFT) & 0xFFFFFFFULL) << 28) ^
                                   (((uint64_t)gx >> DEM_PROVINCE_SHIFT) & 0xFFFFFFFULL));
    const uint32_t k = (uint32_t)((hp >> 33) % 100u);
    const int kind = k < 50u ? 0 : k < 72u ? 1 : 2;                  // mountains, plains, stripes
    const uint64_t hj = splitmix64(seed ^ 0x7700000000000000ULL ^ (((uint64_t)gy & 0xFFFFFFFULL) << 28) ^ ((uint64_t)gx & 0xFFFFFFFULL));
    int64_t sum;
    uint32_t cliffShare, screeShare;                                 // of 64
    if (kind == 0) {
        sum = dem_octaves(seed, gx, gy, 0, 6) + (int64_t)((hj >> 40) % 5) - 2;
        cliffShare = 12; screeShare = 8;
    } else if (kind == 1) {
        sum = (dem_octaves(seed, gx, gy, 0, 1) >> 4) + (int64_t)((hj >> 40) % 13) - 6;
        cliffShare = 0; screeShare = 0;
    } else {
        sum = dem_octaves(seed, gx, gy * 37, 0, 6);
        cliffShare = 4; screeShare = 0;
    }
    const uint64_t hb = splitmix64(seed ^ 0x6600000000000000ULL ^ ((((uint64_t)gy >> 4) & 0xFFFFFFFULL) << 28) ^
                                   (((uint64_t)gx >> 4) & 0xFFFFFFFULL));
    const uint32_t pick = (uint32_t)((hb >> 33) & 63u);
    if (pick < cliffShare) {
        const int64_t i = gx >> 2, j = gy >> 2, fx = gx & 3, fy = gy & 3;
        int64_t l[4];
        for (int q = 0; q < 4; q++) {
            const uint64_t h = splitmix64(seed ^ 0x4400000000000000ULL ^ ((((uint64_t)(j + (q >> 1))) & 0xFFFFFFFULL) << 28) ^
                                          (((uint64_t)(i + (q & 1))) & 0xFFFFFFFULL));
            l[q] = (int64_t)((((h >> 32) & 0xFFFF) * (uint64_t)(2 * DEM_CLIFF_AMP)) >> 16) - DEM_CLIFF_AMP;
        }
        const int64_t top = l[0] * (4 - fx) + l[1] * fx, bot = l[2] * (4 - fx) + l[3] * fx;
        sum += (top * (4 - fy) + bot * fy) >> 4;
    } else if (pick < cliffShare + screeShare) {
        sum += (int64_t)((hj >> 20) % (2u * DEM_SCREE_AMP + 1u)) - (int64_t)DEM_SCREE_AMP;
    }
    sum -= 2000;
    if (sum < -11000) sum = -11000;
    if (sum > 8848) sum = 8848;
    return (int32_t)sum;
}

// ocean mask of the nulls workload: 16 x 16 blocks of the grid, maskPerMille / 1000 of them null
__device__ __forceinline__ bool dem_masked(uint64_t seed, int64_t gx, int64_t gy, int maskPerMille)
{
    const uint64_t h = splitmix64(seed ^ 0x3300000000000000ULL ^ ((((uint64_t)gy >> 4) & 0xFFFFFFFULL) << 28) ^
                                  (((uint64_t)gx >> 4) & 0xFFFFFFFULL));
    return (int)((h >> 33) % 1000u) < maskPerMille;
}

__global__ __launch_bounds__(256) void k_synth_dem(uint64_t seed, int nRows, int nCols, int64_t tilesPerRow,
                                                   int64_t tile0, size_t nTiles, int maskPerMille, int style, int32_t *__restrict__ values)
{
    const size_t nCells = (size_t)nRows * (size_t)nCols;
    const size_t total = nTiles * nCells;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const size_t t = g / nCells;
        const uint32_t k = (uint32_t)(g - t * nCells);
        const int r = (int)(k / (uint32_t)nCols), c = (int)(k - (uint32_t)r * (uint32_t)nCols);
        const int64_t tile = tile0 + (int64_t)t;
        const int64_t tr = tile / tilesPerRow, tc = tile % tilesPerRow;
        const int64_t gx = tc * nCols + c, gy = tr * nRows + r;
        values[g] = maskPerMille > 0 && dem_masked(seed, gx, gy, maskPerMille) ? (int32_t)0x80000000u
                    : style == 1 ? dem_value_rough(seed, gx, gy) : dem_value(seed, gx, gy);
    }
}

}  // namespace

hipError_t gf_launch_compact(size_t nTiles, const uint8_t *slots, size_t slotStride, const uint32_t *lengths,
                             uint64_t *offsets, uint8_t *blob, size_t blobCap, hipStream_t stream, const int32_t *status)
{
    hipLaunchKernelGGL(k_scan_lengths, dim3(1), dim3(1024), 0, stream, nTiles, slotStride, lengths, status, offsets);
    if (nTiles) {
        const unsigned grid = (unsigned)(nTiles < 8192 ? nTiles : 8192);
        hipLaunchKernelGGL(k_gather, dim3(grid), dim3(256), 0, stream, nTiles, slots, slotStride, lengths, status, offsets,
                           blob, blobCap);
    }
    return hipGetLastError();
}

hipError_t gf_launch_synth_dem(uint64_t seed, int nRows, int nCols, int64_t tilesPerRow, int64_t tile0,
                               size_t nTiles, int32_t *values, hipStream_t stream, int maskPerMille, int style)
{
    if (nTiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_synth_dem, dim3(4096), dim3(256), 0, stream, seed, nRows, nCols, tilesPerRow, tile0, nTiles,
                       maskPerMille, style, values);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// CodecCanonHuffman.analyze: the decoder's 256-thread build in analysis mode, then the symbol statistics of its text

namespace {

constexpr int DEC_THREADS = 256;                // = the 256-thread build of gvrs_canon_decode.hip, whose LDS sizes the host passes
constexpr int DEC_WAVES = DEC_THREADS / 64;

#include "gvrs_decode_common.h"

#include "gvrs_canon_decode_common.h"

#include "gvrs_canon_decode_kernel.h"

// ---------------------------------------------------------------------------------------------------------------
// CanonicalHuffman.countSymbols (:352-418), getEntropy (:709-751) and getEscapeBitCountTotal (:656-662) over the text that
// k_canon_decode<true> left of each tile: a workgroup per tile, the tile's nCells values read four at a time.  Byte values
// (nearly all of a terrain tile, most of them 0) go to a replicated 256-bin histogram of their own; the rest -- escapes,
// nulls -- are classified by cn_classify_count and counted into the target bins, count2bit, count8bit and the low-byte
// presence set, with the index expressions of countSymbols (the single 2-bit escape counts count2bit[(s >> 2) & 3]).
// Record per tile (GF_CANON_STAT_WORDS words): bits in the code tables (getBitsInCodeTableCount: the pre-pass record's
// text position less the 48 bits of the header), distinct low bytes (CanonHuffmanStats.addCountsForSymbols), the six
// escape-class counts (2, 4, 6, 8, 16, 24 bits), the escape-bit total (uint64), the entropy (double), 1; all zero where
// the tile has no text to count (a failed decode, the uniform form).
constexpr uint32_t CS_THREADS = 256;
constexpr uint32_t CS_R = 8;                    // replicas of the byte-value histogram (value 0 is most of a terrain tile)

struct CanonStatsLds {
    uint32_t plain[256 * CS_R];                 // symbol value + 128, replica
    uint32_t target[256];                       // target symbols of escaped values
    uint32_t count8[256];
    uint32_t seen[256];                         // low bytes of escaped and null values
    uint32_t count2[4];
    uint32_t cls[8];                            // values per escape kind 1..6, nulls (cn_classify_count)
    uint32_t observed;
    double part[CS_THREADS / 64];
};

__global__ __launch_bounds__(CS_THREADS) void k_canon_stats(const uint32_t *__restrict__ values, const int32_t *__restrict__ status,
                                                           const uint32_t *__restrict__ lengths, const uint32_t *__restrict__ recs,
                                                           uint32_t *__restrict__ out, size_t nTiles, uint32_t nCells)
{
    __shared__ CanonStatsLds L;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    GF_FOR_WG_TILE(t, nTiles) {
        uint32_t *r = out + t * (size_t)GF_CANON_STAT_WORDS;
        if (status[t] != GF_K_OK || lengths[t] <= 6u) {           // analyze throws / the uniform form (counted by the host)
            if (tid < (uint32_t)GF_CANON_STAT_WORDS) r[tid] = 0;
            continue;
        }
        for (uint32_t i = tid; i < 256u * CS_R; i += CS_THREADS) L.plain[i] = 0;
        L.target[tid] = 0;
        L.count8[tid] = 0;
        L.seen[tid] = 0;
        if (tid < 4u) L.count2[tid] = 0;
        if (tid < 8u) L.cls[tid] = 0;
        if (tid == 0) L.observed = 0;
        __syncthreads();

        const uint4 *__restrict__ v4 = reinterpret_cast<const uint4 *>(values + t * (size_t)gf_canon_stats_stride(nCells));
        uint32_t *const h = L.plain + (lane & (CS_R - 1u));
        uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t q = tid; 4u * q < nCells; q += CS_THREADS) {
            const uint4 x4 = v4[q];
            const uint32_t x[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t v = x[j];
                if (4u * q + j >= nCells) break;                   // (the padding of the last four)
                if (v + 128u < 256u) {
                    atomicAdd(h + (v + 128u) * CS_R, 1u);
                    continue;
                }
                const int32_t s = (int32_t)v;
                uint32_t kind;
                const uint32_t target = cn_classify_count(v, &kind);
                L.seen[v & 0xffu] = 1u;
                k[kind]++;
                if (kind == 7u) continue;                          // the null symbol: no target, no escape
                atomicAdd(&L.target[target], 1u);
                if (kind == 1u) atomicAdd(&L.count2[(s >> 2) & 3], 1u);
                if (kind == 2u || kind == 3u) {
                    atomicAdd(&L.count2[(s >> 2) & 3], 1u);
                    atomicAdd(&L.count2[s & 3], 1u);
                }
                if (kind == 3u) atomicAdd(&L.count2[(s >> 4) & 3], 1u);
                if (kind >= 4u) atomicAdd(&L.count8[(s >> 8) & 0xff], 1u);
                if (kind >= 5u) atomicAdd(&L.count8[(s >> 16) & 0xff], 1u);
                if (kind == 6u) atomicAdd(&L.count8[(s >> 24) & 0xff], 1u);
            }
        }
#pragma unroll
        for (int c = 1; c < 8; c++)
            if (k[c]) atomicAdd(&L.cls[c - 1], k[c]);
        __syncthreads();

        // node counts: byte symbols 0..255 (a thread each), null, 1-byte escape, 2-bit escape, end of text (counted once);
        // d = their total = nCells + the escape symbols + 1
        const uint32_t nEsc2 = L.cls[0] + 2u * L.cls[1] + 3u * L.cls[2], nEsc1 = L.cls[3] + 2u * L.cls[4] + 3u * L.cls[5];
        const double d = (double)nCells + (double)nEsc1 + (double)nEsc2 + 1.0;
        uint32_t plainCount = 0;
#pragma unroll
        for (uint32_t m = 0; m < CS_R; m++) plainCount += L.plain[tid * CS_R + m];
        auto plogp = [d](uint32_t n) -> double {
            if (n == 0) return 0.0;
            const double p = (double)n / d;
            return p * log(p);
        };
        double e = plogp(plainCount + L.target[tid]);
        if (tid == 0) e += plogp(L.cls[6]) + plogp(nEsc1) + plogp(nEsc2) + plogp(1u);
        // the escape bits' conditional terms (getEntropy :731-749)
        if (nEsc2 > 0 && tid < 4u && L.count2[tid] > 0) {
            const double q = (double)L.count2[tid] / (double)nEsc2;
            e += ((double)nEsc2 / d) * q * log(q);
        }
        if (nEsc1 > 0 && L.count8[tid] > 0) {
            const double q = (double)L.count8[tid] / (double)nEsc1;
            e += ((double)nEsc1 / d) * q * log(q);
        }
        // distinct low bytes: byte b was seen as the byte value (int8_t)b, i.e. symbol b ^ 0x80, or as the low byte of a wider value
        uint32_t asByte = 0;
#pragma unroll
        for (uint32_t m = 0; m < CS_R; m++) asByte += L.plain[(tid ^ 0x80u) * CS_R + m];
        const bool present = asByte != 0u || L.seen[tid] != 0u;
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) e += __shfl_xor(e, sh, 64);
        const uint32_t nPresent = (uint32_t)__popcll(__ballot(present));
        if (lane == 0) {
            L.part[wave] = e;
            atomicAdd(&L.observed, nPresent);
        }
        __syncthreads();
        if (tid == 0) {
            double sum = 0;
            for (uint32_t w = 0; w < CS_THREADS / 64u; w++) sum += L.part[w];
            const double entropy = -sum / log(2.0);
            const uint64_t escBits = 2ull * L.cls[0] + 4ull * L.cls[1] + 8ull * L.cls[3] + 16ull * L.cls[4] + 24ull * L.cls[5];   // (6-bit class left out, sic)
            uint64_t eb;
            __builtin_memcpy(&eb, &entropy, 8);
            r[0] = recs[t * (size_t)GF_CANON_REC_WORDS + 1] - 48u;
            r[1] = L.observed;
            for (int c = 0; c < 6; c++) r[2 + c] = L.cls[c];
            r[8] = (uint32_t)escBits;
            r[9] = (uint32_t)(escBits >> 32);
            r[10] = (uint32_t)eb;
            r[11] = (uint32_t)(eb >> 32);
            r[12] = 1u;
            r[13] = L.cls[6];
            r[14] = 0;
            r[15] = 0;
        }
        __syncthreads();
    }
}

}  // namespace

// CodecCanonHuffman.analyze of a batch: k_canon_decode<true> (the 256-thread build's LDS sizes in a) behind the code-length pre-pass
// (a.trees), then k_canon_stats over what it left in a.values; the records go to a.analysis
hipError_t gf_launch_canon_analyze(const GfDecodeArgs &a, hipStream_t stream)
{
    if (a.nTiles == 0) return hipSuccess;
    if (!a.trees || !a.analysis) return hipErrorInvalidValue;
    const size_t dyn = (size_t)a.ldsTextBytes + a.ldsStageBytes;
    static GfDynLdsOptIn opt;
    hipError_t e = gf_opt_in_dyn_lds(k_canon_decode<true>, dyn, opt);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_canon_decode<true>, gf_tile_grid(a.nTiles), dim3(DEC_THREADS), dyn, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_canon_stats, gf_tile_grid(a.nTiles), dim3(CS_THREADS), 0, stream, reinterpret_cast<const uint32_t *>(a.values),
                       a.status, a.lengths, a.trees, a.analysis, a.nTiles, (uint32_t)a.nRows * (uint32_t)a.nCols);
    return hipGetLastError();
}
