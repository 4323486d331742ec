// gvrs_crc32c.h -- CRC-32C (Castagnoli, util/GridfourCRC32C.java), the only home of its arithmetic on the host and on the device.
// No HIP header: the file headers include it and tests/csrc/file_*_test.cpp compile them with the host compiler.
//   everywhere: the polynomial, the bit steps, the GF(2) arithmetic that joins checksums, made at compile time where asked
//   the host:   gfCrc32c, eight bytes a step
//   the device: the byte table in LDS, the word steps, and the CRC of a run of words or bytes by a whole wave.  Each lane runs its
//               share through the table and the shares are joined by the CRC's linearity:
//     crc(A || B) = crc(A) * x^(8 |B|)  xor  crc(B)    in GF(2)[x] modulo the (reflected) polynomial,
//               so the whole checksum is the XOR over the lanes of crc(run) * x^(8 bytes behind the run).  The multiplications are
//               32 steps of shift-and-conditional-xor each, the powers by square and multiply.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "gvrs_common.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define GF_CRC_ROLLED _Pragma("unroll 1")                         // device code keeps the 32-step loops as loops
#else
#define GF_CRC_ROLLED
#endif

constexpr uint32_t CRC32C_POLY = 0x82F63B78u;

constexpr GF_HD uint32_t gfCrcBits(uint32_t crc, int nBits)       // nBits zero bits run through the register
{
    for (int k = 0; k < nBits; k++) crc = (crc >> 1) ^ ((crc & 1u) ? CRC32C_POLY : 0u);
    return crc;
}
constexpr GF_HD uint32_t gfCrcTableEntry(uint32_t i) { return gfCrcBits(i, 8); }                 // entry i of the byte table
constexpr GF_HD uint32_t gfCrcWordBits(uint32_t crc, uint32_t w) { return gfCrcBits(crc ^ w, 32); }   // a word without a table

constexpr GF_HD uint32_t gfCrcMulmod(uint32_t a, uint32_t b)      // a * b mod P, operands and result bit-reflected
{
    uint32_t p = 0;
    GF_CRC_ROLLED
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        p ^= (a & m) ? b : 0u;
        b = (b & 1u) ? (b >> 1) ^ CRC32C_POLY : b >> 1;
    }
    return p;
}
template <class N>
constexpr GF_HD uint32_t gfCrcXpow8n(N nBytes)                    // x^(8 nBytes) mod P
{
    uint32_t p = 0x80000000u, sq = 0x00800000u;                   // x^0; x^8
    GF_CRC_ROLLED
    for (N n = nBytes; n; n >>= 1) {
        if (n & 1u) p = gfCrcMulmod(sq, p);
        sq = gfCrcMulmod(sq, sq);
    }
    return p;
}
// crc(A || B) from crc(A), crc(B) and |B| (the arithmetic of zlib's crc32_combine); xpowB = gfCrcXpow8n(|B|)
constexpr GF_HD uint32_t gfCrc32cFold(uint32_t crcA, uint32_t crcB, uint32_t xpowB) { return gfCrcMulmod(xpowB, crcA) ^ crcB; }
constexpr GF_HD uint32_t gfCrc32cCombine(uint32_t crcA, uint32_t crcB, uint64_t lenB) { return gfCrc32cFold(crcA, crcB, gfCrcXpow8n(lenB)); }

// The host's CRC-32C, eight bytes a step through eight byte tables (t[k][b]: byte b followed by k zero bytes): an inspection
// checksums every byte of an image.  (Little-endian hosts, as the library's kernels.)
inline uint32_t gfCrc32c(const uint8_t *p, size_t n)
{
    struct Table {
        uint32_t t[8][256];
        Table()
        {
            for (uint32_t i = 0; i < 256; i++) t[0][i] = gfCrcTableEntry(i);
            for (int k = 1; k < 8; k++)
                for (uint32_t i = 0; i < 256; i++) t[k][i] = t[0][t[k - 1][i] & 0xffu] ^ (t[k - 1][i] >> 8);
        }
    };
    static const Table table;
    const uint32_t(*t)[256] = table.t;
    uint32_t crc = 0xffffffffu;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint32_t a, b;
        memcpy(&a, p + i, 4), memcpy(&b, p + i + 4, 4);
        a ^= crc;
        crc = t[7][a & 0xffu] ^ t[6][(a >> 8) & 0xffu] ^ t[5][(a >> 16) & 0xffu] ^ t[4][a >> 24] ^ t[3][b & 0xffu] ^ t[2][(b >> 8) & 0xffu] ^
              t[1][(b >> 16) & 0xffu] ^ t[0][b >> 24];
    }
    for (; i < n; i++) crc = t[0][(crc ^ p[i]) & 0xffu] ^ (crc >> 8);
    return ~crc;
}

#if defined(__HIPCC__)
// ---- the device: the byte table in LDS ----
// made by a workgroup of 256 threads / by one wave (four entries a lane); both end in the barrier in front of the table's first use
__device__ __forceinline__ void crc_table_fill_256(uint32_t *table)
{
    table[threadIdx.x] = gfCrcTableEntry(threadIdx.x);
    __syncthreads();
}
__device__ __forceinline__ void crc_table_fill_wave(uint32_t *table, uint32_t lane)
{
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) table[lane + 64u * i] = gfCrcTableEntry(lane + 64u * i);
    __syncthreads();
}

__device__ __forceinline__ uint32_t crc_word(const uint32_t *table, uint32_t crc, uint32_t w)
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        crc = table[(crc ^ w) & 0xffu] ^ (crc >> 8);
        w >>= 8;
    }
    return crc;
}
// the whole 16-byte pieces of r[i, end), r + i 4-byte aligned; i ends behind the last one
__device__ __forceinline__ uint32_t crc_pieces16(const uint32_t *table, uint32_t crc, const uint8_t *r, uint32_t &i, uint32_t end)
{
    for (; i + 16u <= end; i += 16u) {
        const GfU4 q = *reinterpret_cast<const GfU4 *>(r + i);
        crc = crc_word(table, crc, q.x);
        crc = crc_word(table, crc, q.y);
        crc = crc_word(table, crc, q.z);
        crc = crc_word(table, crc, q.w);
    }
    return crc;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t part)       // the XOR over the wave's lanes, in every lane
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part ^= gf_lane_xor(part, o);
    return part;
}

// The CRC-32C of n4 words that word(i) delivers, by the whole wave: lane l takes the l-th of 64 runs.  Every lane returns it.
template <class Word>
__device__ __forceinline__ uint32_t wave_crc_words(const uint32_t *table, uint32_t n4, uint32_t lane, Word word)
{
    const uint32_t per = (n4 + 63u) / 64u, begin = min(n4, lane * per), end = min(n4, begin + per);
    uint32_t crc = 0xffffffffu;
    for (uint32_t i = begin; i < end; i++) crc = crc_word(table, crc, word(i));
    crc ^= 0xffffffffu;                                           // the run's own checksum (an empty run: 0)
    return wave_xor(gfCrcMulmod(gfCrcXpow8n(4u * (n4 - end)), crc));
}

// The CRC-32C of r[0, nBytes) by the whole wave: lane l takes the l-th of 64 runs, a multiple of 16 bytes each.  aligned: r is a
// multiple of 4 and is read in 16-byte and 4-byte pieces; byteTail: what is then left of a run -- all of it when r is not aligned --
// is read byte by byte (a caller whose r is always aligned and whose nBytes is a multiple of 4 passes the constants true and
// false, and both branches fold away).  Every lane returns it.
__device__ __forceinline__ uint32_t wave_crc_bytes(const uint32_t *table, const uint8_t *r, uint32_t nBytes, uint32_t lane, bool aligned, bool byteTail)
{
    const uint32_t per = ((nBytes + 63u) / 64u + 15u) & ~15u, begin = min(nBytes, lane * per), end = min(nBytes, begin + per);
    uint32_t crc = 0xffffffffu, i = begin;
    if (aligned) {
        crc = crc_pieces16(table, crc, r, i, end);
        for (; i + 4u <= end; i += 4u) crc = crc_word(table, crc, *reinterpret_cast<const uint32_t *>(r + i));
    }
    if (byteTail)
        for (; i < end; i++) crc = table[(crc ^ r[i]) & 0xffu] ^ (crc >> 8);
    crc ^= 0xffffffffu;                                           // the run's own checksum (an empty run: 0)
    return wave_xor(gfCrcMulmod(gfCrcXpow8n(nBytes - end), crc));
}
#endif
