// lsop_container_test.cpp -- gridfour_amd/csrc/gvrs_lsop_container.h on its own (no HIP, no library): built with the address and
// undefined-behaviour sanitizers and run by tests/test_lsop_container_header.py, which writes the case file and compares what this
// prints with the references.  The case file is what the device encoder leaves for the host, little-endian:
//   u32 family (12 / 8), codec index, rows, columns, flags (GF_LSOP_DEFLATE | GF_LSOP_VALUE_CHECKSUM), tiles; u64 blob capacity;
//   per tile: i32 status, u32 length of the device's packing, those bytes, 16 u32 of the coefficient record, the residuals as i32
// Output: the return value, offsets, types, statuses and the blob's capacity bytes in hex (0xEE where nothing was written).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <zlib.h>

#include "../../gridfour_amd/csrc/gvrs_lsop_container.h"

// (the library's definition, gvrs_api_float.hip)
bool zDeflate(const uint8_t *in, size_t n, int level, std::vector<uint8_t> &out)
{
    uLongf cap = compressBound((uLong)n) + 64;
    out.resize(cap);
    if (compress2(out.data(), &cap, in, (uLong)n, level) != Z_OK) return false;
    out.resize(cap);
    return true;
}

static std::vector<uint8_t> file;
static size_t at = 0;

static void take(void *p, size_t n)
{
    if (at + n > file.size()) {
        printf("case file ends early\n");
        exit(2);
    }
    if (n) memcpy(p, &file[at], n);
    at += n;
}
static uint32_t u32() { uint32_t x; take(&x, 4); return x; }

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + n);
    fclose(f);

    const uint32_t family = u32();
    const int codecIndex = (int)u32(), nRows = (int)u32(), nCols = (int)u32();
    const uint32_t flags = u32();
    const size_t nTiles = u32();
    uint64_t blobCap;
    take(&blobCap, 8);
    if (family != 12 && family != 8) return 2;
    const LsopFamily &F = family == 12 ? GF_LSOP12 : GF_LSOP08;
    if (F.tooSmall(nRows, nCols)) return 2;
    const size_t nRes = F.residualCount(nRows, nCols), resStride = roundUp(nRes, 4), stride = F.maxPacking(nRows, nCols);

    // exactly what the host form brings home: slots of max_packing bytes, records, residuals at their stride
    std::vector<int32_t> st(nTiles), res(nTiles * resStride);
    std::vector<uint32_t> lengths(nTiles), coefs(nTiles * 16);
    std::vector<uint8_t> slots(nTiles * stride, 0xDD);
    for (size_t t = 0; t < nTiles; t++) {
        st[t] = (int32_t)u32();
        lengths[t] = u32();
        if (lengths[t] > stride) {
            printf("tile %zu: %u bytes from the device, max_packing %zu\n", t, lengths[t], stride);
            return 2;
        }
        take(&slots[t * stride], lengths[t]);
        take(&coefs[t * 16], 64);
        take(&res[t * resStride], nRes * 4);
    }
    if (at != file.size()) return 2;

    std::vector<std::vector<uint8_t>> alt;
    lsopAlternatives(F, codecIndex, (flags & GF_LSOP_DEFLATE) != 0, (flags & GF_LSOP_VALUE_CHECKSUM) != 0, nRows, nCols, nTiles, res.data(),
                     resStride, coefs.data(), lengths.data(), st.data(), alt, [](size_t n, auto fn) { for (size_t i = 0; i < n; i++) fn(i); });
    std::vector<uint8_t> blob(blobCap, 0xEE), types(nTiles, 9);      // (the heap: a write past blobCap is the sanitizer's to find)
    std::vector<uint64_t> offsets(nTiles + 1, ~0ull);
    std::vector<int32_t> status(nTiles, 99);
    const gf_status rc = lsopAssemble(F, nTiles, st.data(), lengths.data(), slots.data(), stride, alt, blob.data(), blobCap, offsets.data(),
                                      types.data(), status.data());
    printf("rc %d\noffsets", (int)rc);
    for (uint64_t o : offsets) printf(" %llu", (unsigned long long)o);
    printf("\ntypes");
    for (uint8_t x : types) printf(" %u", x);
    printf("\nstatus");
    for (int32_t x : status) printf(" %d", x);
    printf("\nblob ");
    for (uint8_t x : blob) printf("%02x", x);
    printf("\n");
    return 0;
}
