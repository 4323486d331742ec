// file_inspect_test.cpp -- gvrs_file_inspect.h alone, on the CPU: for every image named on the command line, open it (gfFileParse),
// inspect it and print the verdict (tests/test_file_inspect_program.py compares the line with the restatement's answer), inspect it
// with every room for records and bad tiles below the need (GF_ERR_CAPACITY, the count needed, a guard region untouched), and
// inspect EVERY truncation of the image, each in a heap block of exactly its length so that a read behind it is a fault under the
// address sanitizer: a truncation's records are the whole image's first ones, it never reads as complete with a record cut short,
// and its walk ends inside it.
// Built by tests/test_file_inspect_program.py, plain and with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>

#include "../../gridfour_amd/csrc/gvrs_file_inspect.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static std::vector<uint8_t> readFile(const char *path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static bool sameRecord(const gf_file_record &a, const gf_file_record &b)
{
    return a.pos == b.pos && a.size == b.size && a.type == b.type && a.tile_index == b.tile_index && a.checksum == b.checksum;
}

// ---- the kernels' way to a checksum, step for step on the host: 64 runs of whole 16-byte pieces joined with the table's powers,
// the rest run on behind them (ins_wave_crc), and a large record chunk by chunk with the powers of two (k_inspect_crc_large,
// k_inspect_fold).  What is checked is the arithmetic and the tables, against the plain checksum.
static const GfInspectPowers POWERS = gfInspectMakePowers();

static uint32_t bitCrc(const uint8_t *p, size_t n)                 // the plain checksum, bit by bit
{
    uint32_t crc = 0xffffffffu;
    for (size_t i = 0; i < n; i++) {
        crc ^= p[i];
        for (int b = 0; b < 8; b++) crc = (crc >> 1) ^ ((crc & 1u) ? 0x82F63B78u : 0u);
    }
    return ~crc;
}

static uint32_t waveCrc(const uint8_t *r, uint32_t nBytes)
{
    const uint32_t nFull = nBytes & ~15u, per = ((nFull / 16u + 63u) / 64u) * 16u;
    uint32_t sum = 0;
    for (uint32_t lane = 0; lane < 64; lane++) {
        const uint32_t begin = std::min(nFull, lane * per), end = std::min(nFull, begin + per);
        sum ^= gfCrcMulmod(POWERS.small[(nFull - end) / 16u], end > begin ? gfCrc32c(r + begin, end - begin) : 0u);
    }
    uint32_t crc = ~sum;
    for (uint32_t i = nFull; i < nBytes; i++) {
        crc ^= r[i];
        for (int b = 0; b < 8; b++) crc = (crc >> 1) ^ ((crc & 1u) ? 0x82F63B78u : 0u);
    }
    return ~crc;
}

static uint32_t largeCrc(const uint8_t *r, uint32_t nBytes)
{
    const uint32_t nWhole = nBytes & ~15u;
    uint32_t acc = 0;
    for (uint32_t at = 0; at < nWhole; at += GF_INSPECT_CRC_CHUNK) {
        const uint32_t len = std::min(GF_INSPECT_CRC_CHUNK, nWhole - at);
        uint32_t crc = waveCrc(r + at, len);
        for (uint32_t e = (nWhole - at - len) / 16u, i = 0; e; e >>= 1, i++)
            if (e & 1u) crc = gfCrcMulmod(POWERS.two[i], crc);
        acc ^= crc;
    }
    uint32_t crc = ~acc;
    for (uint32_t i = nWhole; i < nBytes; i++) {
        crc ^= r[i];
        for (int b = 0; b < 8; b++) crc = (crc >> 1) ^ ((crc & 1u) ? 0x82F63B78u : 0u);
    }
    return ~crc;
}

static void checkPowers()
{
    for (uint32_t j = 0; j < GF_INSPECT_SMALL_POWERS; j += (j < 70 ? 1 : 37)) CHECK(POWERS.small[j] == gfCrcXpow8n(16ull * j));
    CHECK(POWERS.small[GF_INSPECT_SMALL_POWERS - 1] == gfCrcXpow8n(16ull * (GF_INSPECT_SMALL_POWERS - 1)));
    for (int i = 0; i < 28; i++) CHECK(POWERS.two[i] == gfCrcXpow8n(16ull << i));
    std::vector<uint8_t> bytes(3 * GF_INSPECT_WAVE_CHUNKS * GF_INSPECT_CRC_CHUNK + 64);
    uint32_t x = 12345;
    for (uint8_t &b : bytes) b = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
    for (uint32_t n = 0; n < 70; n++)                              // the eight-table checksum against the bit-by-bit one, at every phase
        for (uint32_t at = 0; at < 9; at++) CHECK(gfCrc32c(bytes.data() + at, n) == bitCrc(bytes.data() + at, n));
    CHECK(gfCrc32c(bytes.data() + 3, 5001) == bitCrc(bytes.data() + 3, 5001));
    const uint32_t most = GF_INSPECT_WAVE_CHUNKS * GF_INSPECT_CRC_CHUNK;
    for (uint32_t n = 0; n <= most; n += (n < 1100 || n + 40 > most ? 4 : 500)) CHECK(waveCrc(bytes.data(), n) == gfCrc32c(bytes.data(), n));
    for (uint32_t n : {most + 4, most + 12, most + 16, most + GF_INSPECT_CRC_CHUNK, most + GF_INSPECT_CRC_CHUNK + 4, 3 * most - 4, 3 * most, 3 * most + 60})
        CHECK(largeCrc(bytes.data(), n) == gfCrc32c(bytes.data(), n));
}

int main(int argc, char **argv)
{
    checkPowers();
    for (int a = 1; a < argc; a++) {
        const std::vector<uint8_t> image = readFile(argv[a]);
        GfFileParsed p;
        if (image.empty() || gfFileParse(image.data(), image.size(), p) != GF_OK) {
            printf("FAILED to open %s\n", argv[a]);
            return 2;
        }
        gf_file_inspect_report whole;
        CHECK(gfFileInspect(p.info, image.data(), image.size(), &whole, nullptr, 0, nullptr, 0) == GF_OK);
        const size_t n = (size_t)whole.n_records, nBad = (size_t)whole.n_bad_tiles;
        std::vector<gf_file_record> records(n + 2);
        std::vector<int32_t> bad(nBad + 2, 0x7f7f7f7f);
        gf_file_inspect_report r;
        CHECK(gfFileInspect(p.info, image.data(), image.size(), &r, bad.data(), nBad, records.data(), n) == GF_OK);
        CHECK(memcmp(&r, &whole, sizeof(r)) == 0 && bad[nBad] == 0x7f7f7f7f);
        uint64_t byType = 0;
        for (int k = 0; k < 7; k++) byType += whole.n_by_type[k];
        CHECK(byType == n - (whole.stop == GF_INSPECT_BAD_RECORD_TYPE ? 1 : 0));
        CHECK(whole.termination_pos <= image.size() && whole.complete == (whole.stop == GF_INSPECT_END));
        for (size_t k = 0; k + 1 < n; k++) CHECK(records[k].pos + records[k].size == records[k + 1].pos);
        if (n) CHECK(records[0].pos == p.info.content_pos);
        // every room below the need
        for (size_t cap = 0; cap < n; cap++) {
            std::vector<gf_file_record> few(cap + 1);
            memset(few.data(), 0x7f, (cap + 1) * sizeof(gf_file_record));
            gf_file_record guard;
            memset(&guard, 0x7f, sizeof(guard));
            CHECK(gfFileInspect(p.info, image.data(), image.size(), &r, nullptr, 0, few.data(), cap) == GF_ERR_CAPACITY);
            CHECK(r.status == GF_ERR_CAPACITY && r.n_records == n && memcmp(&few[cap], &guard, sizeof(guard)) == 0);
            for (size_t k = 0; k < cap; k++) CHECK(sameRecord(few[k], records[k]));
        }
        for (size_t cap = 0; cap < nBad; cap++) {
            std::vector<int32_t> few(cap + 1, 0x7f7f7f7f);
            CHECK(gfFileInspect(p.info, image.data(), image.size(), &r, few.data(), cap, nullptr, 0) == GF_OK);
            CHECK(r.n_bad_tiles == nBad && few[cap] == 0x7f7f7f7f && memcmp(few.data(), bad.data(), cap * 4) == 0);
        }
        // every truncation, in a block of exactly its length
        size_t walked = 0;
        std::vector<gf_file_record> part(n + 2);
        for (size_t len = 0; len < image.size(); len++) {
            uint8_t *exact = (uint8_t *)malloc(len ? len : 1);
            memcpy(exact, image.data(), len);
            const gf_status s = gfFileInspect(p.info, exact, len, &r, bad.data(), nBad, part.data(), n + 2);
            if (len < p.info.content_pos) CHECK(s == GF_ERR_ARG);
            else {
                walked++;
                CHECK(s == GF_OK && r.termination_pos <= len && r.n_records <= n);
                const size_t m = (size_t)r.n_records;
                // the records in front of the cut are the whole image's; the one the cut falls into stops the walk
                for (size_t k = 0; k + 1 < m; k++) CHECK(sameRecord(part[k], records[k]));
                if (m && part[m - 1].pos + part[m - 1].size > len && r.stop != GF_INSPECT_BAD_RECORD_SIZE && r.stop != GF_INSPECT_BAD_RECORD_TYPE &&
                    r.stop != GF_INSPECT_BAD_TILE_INDEX && r.stop != GF_INSPECT_TILE_TOO_LARGE)
                    CHECK(r.stop == GF_INSPECT_TRUNCATED && !r.complete && r.failed);
                if (r.complete) CHECK(len - r.termination_pos <= 12 || whole.termination_pos == r.termination_pos);
            }
            free(exact);
        }
        printf("%s: %zu bytes, %zu records, stop %d, failed %d, complete %d, dir %d, end %llu, %zu bad, %llu failures, %zu truncations walked\n", argv[a],
               image.size(), n, whole.stop, whole.failed, whole.complete, whole.tile_dir_passed, (unsigned long long)whole.termination_pos, nBad,
               (unsigned long long)whole.n_checksum_failures, walked);
    }
    printf(failures ? "FAILED %d\n" : "done\n", failures);
    return failures ? 1 : 0;
}
