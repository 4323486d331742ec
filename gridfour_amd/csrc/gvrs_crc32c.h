// gvrs_crc32c.h -- CRC-32C (Castagnoli, util/GridfourCRC32C.java) arithmetic shared by the kernels that compute one with a whole
// wave: k_lsop_value_crc (gvrs_lsop.hip) and k_record_crc32c_elems (gvrs_records.hip).  Each lane runs its share of the bytes through
// the polynomial's byte table (in LDS, made by the workgroup) and the shares are joined by the CRC's linearity:
//   crc(A || B) = crc(A) * x^(8 |B|)  xor  crc(B)    in GF(2)[x] modulo the (reflected) polynomial,
// so the whole checksum is the XOR over the lanes of crc(run) * x^(8 bytes behind the run).  The multiplications are 32 steps of
// shift-and-conditional-xor each, the powers by square and multiply.
#pragma once

#include <stdint.h>

constexpr uint32_t CRC32C_POLY = 0x82F63B78u;
__device__ __forceinline__ uint32_t crc_mulmod(uint32_t a, uint32_t b)        // a * b mod P, operands and result bit-reflected
{
    uint32_t p = 0;
#pragma unroll 1
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        p ^= (a & m) ? b : 0u;
        b = (b & 1u) ? (b >> 1) ^ CRC32C_POLY : b >> 1;
    }
    return p;
}
__device__ __forceinline__ uint32_t crc_xpow8n(uint32_t nBytes)               // x^(8 nBytes) mod P
{
    uint32_t p = 0x80000000u, sq = 0x00800000u;                               // x^0; x^8
#pragma unroll 1
    for (uint32_t n = nBytes; n; n >>= 1) {
        if (n & 1u) p = crc_mulmod(sq, p);
        sq = crc_mulmod(sq, sq);
    }
    return p;
}
// entry i of the byte table, for thread i of a workgroup of at least 256 threads
__device__ __forceinline__ uint32_t crc_table_entry(uint32_t i)
{
    uint32_t c = i;
#pragma unroll
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? CRC32C_POLY : 0u);
    return c;
}
