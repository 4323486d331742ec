// file_update_test.cpp -- gvrs_file_update.h alone, on the CPU: for every image named on the command line, open it (gfFileParse),
// begin an update, close it again without a record (a file without free space must come back byte for byte),
// update it with records made here in three orders, with every image_cap below the need (GF_ERR_CAPACITY and not one byte
// changed, checked with a guard region), update the updated image again, and run begin and assemble over EVERY truncation of the
// image, each in a buffer of exactly its length so that a read behind it is a fault under the address sanitizer.
// Built by tests/test_file_update_program.py, plain and with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>

#include "../../gridfour_amd/csrc/gvrs_file_update.h"

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

// a tile record of `size` bytes for one element
static void appendRecord(std::vector<uint8_t> &blob, int32_t tile, size_t size, bool checksums)
{
    const size_t start = blob.size();
    GfFileOut o(blob);
    o.zeros(8);
    o.i32(tile);
    o.i32((int32_t)(size - 20));
    for (size_t k = 0; k < size - 20; k++) o.u8((int)((tile * 5 + k) & 0xff));
    gfFileCloseRecord(blob, start, GF_FILE_REC_TILE, checksums);
}

// every record tiles the image from the content position to its end
static bool tiles(const std::vector<uint8_t> &image, uint64_t contentPos)
{
    uint64_t at = contentPos;
    while (at < image.size()) {
        if (image.size() - at < 16) return false;
        const uint64_t size = gfLe(image.data() + at, 4);
        if (size < 16 || (size & 7) != 0 || size > image.size() - at) return false;
        at += size;
    }
    return at == image.size();
}

static gf_status update(const std::vector<uint8_t> &image, const std::vector<int32_t> &tilesIn, const std::vector<size_t> &sizes, int64_t time,
                        std::vector<uint8_t> &out)
{
    GfFileParsed p;
    gf_status s = gfFileParse(image.data(), image.size(), p);
    if (s != GF_OK) return s;
    GfFileUpdate u;
    if ((s = gfFileUpdateBegin(p.info, image.data(), image.size(), u)) != GF_OK) return s;
    std::vector<uint8_t> blob;
    std::vector<uint64_t> offsets(1, 0);
    for (size_t k = 0; k < tilesIn.size(); k++) {
        if (sizes[k]) appendRecord(blob, tilesIn[k], sizes[k], p.info.checksum_enabled != 0);
        offsets.push_back(blob.size());
    }
    blob.resize(blob.size() + 1);                                  // (never empty: data() is a pointer)
    uint64_t need = 0, need2 = 0;
    out = image;
    s = gfFileUpdateAssemble(u, out.data(), out.size(), blob.data(), offsets.data(), tilesIn.data(), nullptr, tilesIn.size(), time, 0, &need);
    if (s != GF_ERR_CAPACITY) return s;
    CHECK(out == image && need > image.size());
    // every capacity below the need, in steps of 8: refused, the image and the guard behind it unchanged
    for (uint64_t cap = image.size(); cap < need; cap += 8) {
        std::vector<uint8_t> buf((size_t)cap, 0xA5);
        memcpy(buf.data(), image.data(), image.size());
        const std::vector<uint8_t> before(buf);
        CHECK(gfFileUpdateAssemble(u, buf.data(), cap, blob.data(), offsets.data(), tilesIn.data(), nullptr, tilesIn.size(), time, 0, &need2) == GF_ERR_CAPACITY);
        CHECK(need2 == need && buf == before);
    }
    out.assign((size_t)need, 0xA5);
    memcpy(out.data(), image.data(), image.size());
    s = gfFileUpdateAssemble(u, out.data(), out.size(), blob.data(), offsets.data(), tilesIn.data(), nullptr, tilesIn.size(), time, 0, &need2);
    CHECK(need2 == need);
    return s;
}

int main(int argc, char **argv)
{
    // the serial rules on a list of their own
    {
        uint64_t pos[8], size[8], fileSize = 1000;
        uint32_t n = 0;
        CHECK(gfFsDealloc(pos, size, n, 8, 200, 64) && gfFsDealloc(pos, size, n, 8, 400, 64) && n == 2);
        CHECK(gfFsDealloc(pos, size, n, 8, 264, 136) && n == 1 && pos[0] == 200 && size[0] == 264);      // the prior, then the next
        CHECK(gfFsAlloc(pos, size, n, fileSize, 240) == 1000 && fileSize == 1240 && n == 1);             // larger by 24: skipped, appended
        CHECK(gfFsAlloc(pos, size, n, fileSize, 232) == 200 && n == 1 && pos[0] == 432 && size[0] == 32);
        CHECK(gfFsAlloc(pos, size, n, fileSize, 32) == 432 && n == 0);
        CHECK(gfFsDealloc(pos, size, n, 8, 1200, 40) && gfFsAlloc(pos, size, n, fileSize, 48) == 1200 && fileSize == 1248 && n == 0);
        uint32_t full = 0;
        CHECK(!gfFsDealloc(pos, size, full, 0, 8, 8));
    }
    for (int a = 1; a < argc; a++) {
        const std::vector<uint8_t> image = readFile(argv[a]);
        GfFileParsed p;
        if (image.empty() || gfFileParse(image.data(), image.size(), p) != GF_OK) {
            printf("FAILED to open %s\n", argv[a]);
            return 2;
        }
        const int64_t time = (int64_t)gfLe(image.data() + GF_FILE_POS_TIME_MODIFIED, 8);
        std::vector<uint8_t> out, again;
        CHECK(update(image, {}, {}, time, out) == GF_OK && tiles(out, p.info.content_pos));
        if (p.info.freespace_dir_pos == 0) CHECK(out == image);   // (a file without free space closes as it was)
        const gf_grid_spec &g = p.info.grid;
        const int32_t nTiles = (int32_t)((((int64_t)g.n_rows_grid + g.n_rows_tile - 1) / g.n_rows_tile) * (((int64_t)g.n_cols_grid + g.n_cols_tile - 1) / g.n_cols_tile));
        if (p.info.n_codecs > 0 && nTiles >= 4) {                  // (a file without compression takes only records of its own size)
            const std::vector<std::vector<int32_t>> orders = {{0, 1, 2, 3}, {3, 2, 1, 0}, {2, 0, 3, 1}};
            for (const std::vector<int32_t> &order : orders) {
                std::vector<size_t> sizes;
                for (const int32_t t : order) sizes.push_back(t == 1 ? 0 : 24 + 40 * (size_t)t);
                CHECK(update(image, order, sizes, time + 1, out) == GF_OK && tiles(out, p.info.content_pos));
                GfFileParsed q;
                CHECK(gfFileParse(out.data(), out.size(), q) == GF_OK);
                CHECK(update(out, {nTiles - 1, 0}, {64, 0}, time + 2, again) == GF_OK && tiles(again, p.info.content_pos));
            }
        }
        // every truncation, in a buffer of exactly its length
        size_t opened = 0;
        for (size_t n = 0; n < image.size(); n++) {
            uint8_t *exact = (uint8_t *)malloc(n ? n : 1);
            memcpy(exact, image.data(), n);
            GfFileParsed q;
            GfFileUpdate u;
            if (gfFileParse(exact, n, q) == GF_OK && gfFileUpdateBegin(q.info, exact, n, u) == GF_OK) {
                opened++;
                uint64_t need = 0;
                const uint64_t none[1] = {0};
                (void)gfFileUpdateAssemble(u, exact, n, nullptr, none, nullptr, nullptr, 0, time, 0, &need);
            }
            free(exact);
        }
        printf("%s: %zu bytes, %zu truncations opened\n", argv[a], image.size(), opened);
    }
    printf(failures ? "FAILED %d\n" : "done\n", failures);
    return failures ? 1 : 0;
}
