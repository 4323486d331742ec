// gvrs_lsop_container.h -- what LSOP12 and LSOP08 share above their kernels: the table of the two families' numbers and the host's
// half of the encoders (lsop/LsEncoder12.java:180-216, LsEncoder08.java:83-134): CodecM32 bytes of the two residual streams, zlib,
// the Deflate container, the choice between it and the device's packing, and the blob of a batch.  Host arithmetic on bytes: no HIP
// header, so that tests/csrc/lsop_container_test.cpp runs it under the sanitizers on any machine.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/gvrs_hip_codec.h"
#include "gvrs_common.h"

#pragma GCC visibility push(hidden)          // nothing here is an export of the library

inline size_t roundUp(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline void putLE32(uint8_t *p, uint32_t x) { p[0] = (uint8_t)x; p[1] = (uint8_t)(x >> 8); p[2] = (uint8_t)(x >> 16); p[3] = (uint8_t)(x >> 24); }

// zlib stream of n bytes at a level (defined in gvrs_api_float.hip; the test program brings its own copy)
bool zDeflate(const uint8_t *in, size_t n, int level, std::vector<uint8_t> &out);

// How the host chooses between the device's packing and the Deflate container
enum LsopChoice {
    // LsEncoder12.java:180-216: the interior stream first; zlib failing, an empty stream, one longer than its input + 128 or a sum
    // that is not strictly smaller than the device's body silently keep the device's packing
    LSOP_DEFLATE_IF_SMALLER,
    // LsEncoder08.java:83-134: both streams; zlib failing or a stream longer than its input + 128 (the reference's buffer, which it
    // would silently cut) is GF_ERR_UNSUPPORTED; the device's packing is kept only where its body is STRICTLY shorter (:118)
    LSOP_DEVICE_IF_SMALLER,
};

struct LsopFamily {
    uint32_t nCoef;                         // coefficients of the predictor; a tile's 16-word record: seed, nCoef floats, spare words
    int minSide;                            // fewer rows or columns: LsOptimalPredictor12.java:114-116, 08.java:62-64 -> null
    int initPerRow, initPerCol, initLess;   // initialisers: initPerRow * nRows + initPerCol * nCols - initLess
    int interiorColsLess;                   // interior: (nRows - 2) * (nCols - interiorColsLess)
    size_t hdrDevice[2], hdrDeflate[2];     // header bytes of the device's container and of the Deflate one, without / with value checksum
    size_t maxTables, maxBitsPerValue, maxTailBits;   // max_packing: the largest header + 2 * maxTables + the residuals' bits + 16
    bool maxZeroWhenSmall;                  // ... and 0 for a tile that is too small
    int typeDevice;                         // container type the device encoder writes (the Deflate container is type 1)
    LsopChoice choice;
    int maxCols;                            // shape limit: more columns, or maxCells cells or more, are GF_ERR_UNSUPPORTED
    uint64_t maxCells;
    bool hostFormsCheckShape;               // the host forms refuse such a shape before they stage (LSOP12's leave it to its predictor)

    bool tooSmall(int nRows, int nCols) const { return nRows < minSide || nCols < minSide; }
    bool tooLarge(int nRows, int nCols) const { return nCols > maxCols || (uint64_t)nRows * (uint64_t)nCols >= maxCells; }
    size_t nInit(int nRows, int nCols) const { return (size_t)initPerRow * nRows + (size_t)initPerCol * nCols - initLess; }
    size_t nInt(int nRows, int nCols) const { return (size_t)(nRows - 2) * (size_t)(nCols - interiorColsLess); }
    size_t residualCount(int nRows, int nCols) const { return tooSmall(nRows, nCols) ? 0 : nInit(nRows, nCols) + nInt(nRows, nCols); }
    size_t maxPacking(int nRows, int nCols) const
    {
        const size_t n = residualCount(nRows, nCols);
        if (n == 0 && maxZeroWhenSmall) return 0;
        return roundUp(hdrDevice[1] + 2 * maxTables + (n * maxBitsPerValue + maxTailBits) / 8 + 16, 16);
    }
};

// LSOP12, canonical Huffman from the device: 55 header bytes (59 with the value checksum) + two streams (tables < 750 bytes each, at
// most 84 bits per value + end-of-text).  The predictor takes fewer than 2^28 cells.
constexpr LsopFamily GF_LSOP12 = {12, 6, 4, 2, 9, 4, {55, 59}, {63, 67}, 768, 84, 2 * 15 + 7, false, 2, LSOP_DEFLATE_IF_SMALLER,
                                  INT32_MAX, 1ull << 28, false};
// LSOP08, Huffman of M32 bytes from the device: 47 header bytes + two bodies.  A serialised tree is at most 8 + 10 * 256 - 1 bits and
// the text no longer than the M32 bytes themselves (a Huffman code of at most 256 symbols is never longer than the fixed 8-bit one);
// Deflate: each zlib stream has at most its input's length + 128.  A value has at most 6 M32 bytes.  k_lsop8_reconstruct keeps two
// rows of a tile in LDS (GF_LSOP8_MAX_COLS columns); the packer counts a packing's bits in 32 bits.
constexpr LsopFamily GF_LSOP08 = {8, 4, 2, 2, 5, 2, {47, 47}, {47, 47}, 328, 48, 0, true, 0, LSOP_DEVICE_IF_SMALLER,
                                  16384, 1ull << 26, true};

// CodecM32.encode (compress/CodecM32.java:257-311) of a residual array
inline size_t m32Pack(const int32_t *x, size_t n, std::vector<uint8_t> &out)
{
    out.resize(6 * n + 8);
    size_t k = 0;
    for (size_t i = 0; i < n; i++) {
        const int len = gf_m32_len((uint32_t)x[i]);
        for (int b = 0; b < len; b++) out[k++] = (uint8_t)gf_m32_byte((uint32_t)x[i], len, b);
    }
    out.resize(k);
    return k;
}

// LsHeader.packHeader of a Deflate container: codec index, COMPRESSION_TYPE_DEFLATE | REVISION_FLAG (| VALUE_CHECKSUM_INCLUDED), the
// coefficient count, seed and coefficients from the tile's record, the two M32 byte counts, the checksum (the record's word behind
// the coefficients, :259-261).  p has F.hdrDeflate[valueChecksum] bytes.
inline void lsopDeflateHeader(const LsopFamily &F, int codecIndex, bool valueChecksum, const uint32_t *record, size_t nMI, size_t nMX, uint8_t *p)
{
    p[0] = (uint8_t)codecIndex;
    p[1] = valueChecksum ? 0xC1 : 0x41;
    p[2] = (uint8_t)F.nCoef;
    uint8_t *q = p + 3;
    for (uint32_t k = 0; k <= F.nCoef; k++, q += 4) putLE32(q, record[k]);
    putLE32(q, (uint32_t)nMI);
    putLE32(q + 4, (uint32_t)nMX);
    if (valueChecksum) putLE32(q + 8, record[F.nCoef + 1]);
}

// One tile the device encoded: residuals (initialisers, then interior), its record and the length of its packing -> alt, the Deflate
// container where the family's rule prefers it (left empty otherwise), and the tile's status.
inline gf_status lsopAlternative(const LsopFamily &F, int codecIndex, bool valueChecksum, int nRows, int nCols, const int32_t *residuals,
                                 const uint32_t *record, size_t deviceLength, std::vector<uint8_t> &alt)
{
    const size_t nInit = F.nInit(nRows, nCols), nInt = F.nInt(nRows, nCols), deviceBody = deviceLength - F.hdrDevice[valueChecksum];
    std::vector<uint8_t> mInit, mInt, zInit, zInt;
    const size_t nMX = m32Pack(residuals + nInit, nInt, mInt);
    size_t nMI;
    if (F.choice == LSOP_DEFLATE_IF_SMALLER) {
        if (!zDeflate(mInt.data(), nMX, 6, zInt)) return GF_OK;
        if (zInt.empty() || zInt.size() >= deviceBody || zInt.size() > nMX + 128) return GF_OK;                      // :185-187
        nMI = m32Pack(residuals, nInit, mInit);
        if (!zDeflate(mInit.data(), nMI, 6, zInit)) return GF_OK;
        if (zInit.empty() || zInit.size() + zInt.size() >= deviceBody || zInit.size() > nMI + 128) return GF_OK;     // :194-196
    } else {
        nMI = m32Pack(residuals, nInit, mInit);
        if (!zDeflate(mInit.data(), nMI, 6, zInit) || !zDeflate(mInt.data(), nMX, 6, zInt) || zInit.size() > nMI + 128 ||
            zInt.size() > nMX + 128)
            return GF_ERR_UNSUPPORTED;
        if (deviceBody < zInit.size() + zInt.size()) return GF_OK;
    }
    const size_t hdr = F.hdrDeflate[valueChecksum];
    alt.resize(hdr + zInit.size() + zInt.size());
    lsopDeflateHeader(F, codecIndex, valueChecksum, record, nMI, nMX, alt.data());
    memcpy(&alt[hdr], zInit.data(), zInit.size());
    memcpy(&alt[hdr + zInit.size()], zInt.data(), zInt.size());
    return GF_OK;
}

// ... for every tile of a batch whose status is GF_OK (status[t] becomes the tile's).  forEach(n, f) calls f(0 .. n - 1), in any order
// and on any threads.  Without deflate nothing is done: every tile keeps the device's packing.
template <class ForEach>
inline void lsopAlternatives(const LsopFamily &F, int codecIndex, bool deflate, bool valueChecksum, int nRows, int nCols, size_t nTiles,
                             const int32_t *residuals, size_t resStride, const uint32_t *records, const uint32_t *lengths, int32_t *status,
                             std::vector<std::vector<uint8_t>> &alt, ForEach forEach)
{
    alt.assign(nTiles, std::vector<uint8_t>());
    if (!deflate) return;
    forEach(nTiles, [&](size_t t) {
        if (status[t] == GF_OK)
            status[t] = lsopAlternative(F, codecIndex, valueChecksum, nRows, nCols, residuals + t * resStride, records + t * 16, lengths[t], alt[t]);
    });
}

// The batch's answer: offsets[nTiles + 1], types and status (either may be null) and, when it fits, the blob of the winners laid back
// to back.  GF_ERR_CAPACITY leaves the blob untouched, with everything else written (offsets[nTiles] = the bytes needed).
inline gf_status lsopAssemble(const LsopFamily &F, size_t nTiles, const int32_t *st, const uint32_t *lengths, const uint8_t *slots, size_t slotStride,
                              const std::vector<std::vector<uint8_t>> &alt, uint8_t *blob, size_t blobCap, uint64_t *offsets, uint8_t *types,
                              int32_t *status)
{
    uint64_t total = 0;
    for (size_t t = 0; t < nTiles; t++) {
        offsets[t] = total;
        if (st[t] == GF_OK) total += alt[t].empty() ? lengths[t] : alt[t].size();
        if (types) types[t] = (uint8_t)(st[t] != GF_OK ? 0 : alt[t].empty() ? F.typeDevice : 1);
    }
    offsets[nTiles] = total;
    if (status) memcpy(status, st, nTiles * 4);
    if (total > blobCap) return GF_ERR_CAPACITY;
    for (size_t t = 0; t < nTiles; t++) {
        if (st[t] != GF_OK) continue;
        if (alt[t].empty()) memcpy(blob + offsets[t], slots + t * slotStride, lengths[t]);
        else memcpy(blob + offsets[t], alt[t].data(), alt[t].size());
    }
    return GF_OK;
}

#pragma GCC visibility pop
