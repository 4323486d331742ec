// gvrs_blocks_common.h -- what the grid-block kernels share (gvrs_blocks.hip: gather and cut; gvrs_blocks_write.hip: the cut of a
// block write): the workgroup size, the row routine that moves a run of cells as 16-byte pieces aligned on the destination, and the
// number of lanes a row gets.  Device code only; every function is inlined into its kernel.
// NOTE: bw_pieces / bw_row of gvrs_blocks_write.hip are copies of blk_pieces / blk_row<false> below with a per-piece hook between load
// and store (kept apart so that the three kernels of gvrs_blocks.hip keep their code): a change to the row scheme -- head, body and
// tail arithmetic, pieces per lane -- has to be made in both places.
#pragma once

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"

namespace {

constexpr uint32_t BLK_THREADS = 256;

__device__ __forceinline__ int64_t blk_max(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ __forceinline__ int64_t blk_min(int64_t a, int64_t b) { return a < b ? a : b; }

// the fill value as a word (a SHORT's 16 bits twice)
__device__ __forceinline__ uint32_t blk_fill_word(uint32_t fillBits, uint32_t itemBytes)
{
    return itemBytes == 2u ? (fillBits & 0xffffu) * 0x10001u : fillBits;
}

// nPieces pieces of type T (GfU4: 16 bytes, aligned on the destination, the source 4-byte aligned; uint16_t: a halfword) from src to
// dst, or the value `fill` instead (FILL); piece p by lane p mod L of the row's L lanes.  Four pieces per lane are loaded, then
// stored; every store instruction writes L consecutive pieces; a row of more than 4 L pieces is looped over.
template <class T, bool FILL>
__device__ __forceinline__ void blk_pieces(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nPieces, uint32_t l, uint32_t L,
                                           const T fill)
{
    T *__restrict__ d = reinterpret_cast<T *>(dst);
    const T *__restrict__ s = reinterpret_cast<const T *>(src);
#pragma unroll 1
    for (uint32_t p = l; p < nPieces; p += 4u * L) {
        const uint32_t p1 = p + L, p2 = p + 2u * L, p3 = p + 3u * L;
        T v0 = fill, v1 = fill, v2 = fill, v3 = fill;
        if (!FILL) {
            v0 = s[p];
            if (p1 < nPieces) v1 = s[p1];
            if (p2 < nPieces) v2 = s[p2];
            if (p3 < nPieces) v3 = s[p3];
        }
        d[p] = v0;
        if (p1 < nPieces) d[p1] = v1;
        if (p2 < nPieces) d[p2] = v2;
        if (p3 < nPieces) d[p3] = v3;
    }
}

// one cell (2 or 4 bytes) at byte offset `at`
template <bool FILL>
__device__ __forceinline__ uint32_t blk_cell_load(const uint8_t *__restrict__ src, uint32_t at, uint32_t itemBytes, uint32_t fillWord)
{
    if (FILL) return fillWord;
    return itemBytes == 2u ? (uint32_t) * reinterpret_cast<const uint16_t *>(src + at) : *reinterpret_cast<const uint32_t *>(src + at);
}
__device__ __forceinline__ void blk_cell_store(uint8_t *__restrict__ dst, uint32_t at, uint32_t itemBytes, uint32_t v)
{
    if (itemBytes == 2u) *reinterpret_cast<uint16_t *>(dst + at) = (uint16_t)v;
    else *reinterpret_cast<uint32_t *>(dst + at) = v;
}

// One row run of nBytes (a multiple of itemBytes; dst and src aligned to itemBytes) by the L lanes of its row group, l = the lane's
// number among them, L a power of two >= 8.  Where the two sides agree modulo 4 -- always for 4-byte items -- the piece is 16 bytes,
// aligned on the destination: where they agree modulo 16 too the load is aligned as well, otherwise it is a 16-byte load at a
// 4-byte aligned address (GfU4), which gfx950 serves: a quarter of the instructions of a word-by-word copy of such a row.
// A SHORT row whose sides disagree modulo 4 goes halfword by halfword.  The cells in front of the first and behind the last piece
// (fewer than 16 / itemBytes <= 8 each) go one per lane.  FILL: the fill value instead of a source.
template <bool FILL>
__device__ __forceinline__ void blk_row(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t nBytes, uint32_t itemBytes, uint32_t fillWord,
                                        uint32_t l, uint32_t L)
{
    if (nBytes == 0u) return;
    if (FILL) src = dst;                                                       // (never read)
    const uint32_t diff = FILL ? 0u : (uint32_t)((uintptr_t)dst - (uintptr_t)src);
    const uint32_t unit = (diff & 3u) == 0u ? 16u : 2u;
    uint32_t head = (uint32_t)(0u - (uint32_t)(uintptr_t)dst) & (unit - 1u);
    if (head > nBytes) head = nBytes;
    const uint32_t nBody = (nBytes - head) / unit, tail0 = head + nBody * unit;
    const bool hasHead = l * itemBytes < head, hasTail = tail0 + l * itemBytes < nBytes;
    uint32_t hv = 0, tv = 0;
    if (hasHead) hv = blk_cell_load<FILL>(src, l * itemBytes, itemBytes, fillWord);
    if (hasTail) tv = blk_cell_load<FILL>(src, tail0 + l * itemBytes, itemBytes, fillWord);
    if (unit == 16u) {
        GfU4 f;
        f.x = f.y = f.z = f.w = fillWord;
        blk_pieces<GfU4, FILL>(dst + head, src + head, nBody, l, L, f);
    } else blk_pieces<uint16_t, FILL>(dst + head, src + head, nBody, l, L, (uint16_t)fillWord);
    if (hasHead) blk_cell_store(dst, l * itemBytes, itemBytes, hv);
    if (hasTail) blk_cell_store(dst, tail0 + l * itemBytes, itemBytes, tv);
}

// lanes per row group, as a shift: the smallest power of two, 8 .. 256, with which four pieces per lane (blk_pieces: four loads in
// flight) cover a row's 16-byte pieces and its two ends
__device__ __forceinline__ uint32_t blk_row_lanes_log2(uint32_t rowBytes)
{
    const uint32_t pieces = rowBytes / 16u + 2u;
    uint32_t s = 3u;
    while ((4u << s) < pieces && s < 8u) s++;
    return s;
}

}  // namespace
