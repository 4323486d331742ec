// file_parse_test.cpp -- gvrs_file_parse.h alone, under the sanitizers: the reference's sample files, every prefix of them and
// single-byte changes of every byte of their header region through the parser and the directory look-up.  Every image is a heap
// block of exactly its length, so that a read at or behind image_bytes is a report.  First, with no file: the directory's shared
// rules (entry of a tile, tile of an entry, an entry's position, the place rule) against tables written out by hand.
//   file_parse_test FILE...      prints one line per file: the facts the Python test compares; exit 0, or 1 with a message
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gridfour_amd/csrc/gvrs_file_parse.h"

static int fail(const char *path, const char *what, long at)
{
    printf("FAIL %s: %s at %ld\n", path, what, at);
    return 1;
}

// parse and look every tile up: what a reader does with an image
static gf_status openAndLocate(const uint8_t *image, size_t n, uint64_t *sum)
{
    GfFileParsed p;
    const gf_status s = gfFileParse(image, n, p);
    if (s != GF_OK) return s;
    const GfFileDir d = gfFileDirOf(p.info);
    const gf_grid_spec &g = p.info.grid;
    const int64_t nTiles = (int64_t)d.nColsOfTiles * (((int64_t)g.n_rows_grid + g.n_rows_tile - 1) / g.n_rows_tile);
    for (int64_t t = 0; t < nTiles && t < 4096; t++) {
        uint64_t pos;
        uint32_t size;
        (void)gfFileLocate(d, image, n, (int32_t)t, &pos, &size);
        *sum += pos + size;
    }
    return GF_OK;
}

// The rules every reader of a tile directory shares, against tables written out by hand: a 2 x 3 directory at tile row 1, tile
// column 2 of a grid of 4 x 6 tiles, compact and extended, its image cut at every length from the first entry's start to one byte
// behind the last entry's end (each in a block of its own length), and the place rule clause by clause.
static int rulesTable()
{
    static const int entryOfTile[24] = {-1, -1, -1, -1, -1, -1, -1, -1, 0, 1, 2, -1, -1, -1, 3, 4, 5, -1, -1, -1, -1, -1, -1, -1};
    static const int tileOfEntry[6] = {8, 9, 10, 14, 15, 16};
    static const uint8_t compact[24] = {5, 0, 0, 0, 0, 0, 0, 0, 7, 0, 0, 0, 9, 0, 0, 0, 0xff, 0xff, 0xff, 0xff, 11, 0, 0, 0};
    static const uint8_t extended[48] = {40, 0, 0, 0, 0, 0, 0, 0, 0,    0,    0,    0,    0,    0,    0,    0,    56, 0, 0, 0, 0, 0, 0, 0,
                                         72, 0, 0, 0, 0, 0, 0, 0, 0xf0, 0xde, 0xbc, 0x9a, 0x78, 0x56, 0x34, 0x12, 88, 0, 0, 0, 0, 0, 0, 0};
    static const uint64_t posCompact[6] = {40, 0, 56, 72, 0x7fffffff8ull, 88}, posExtended[6] = {40, 0, 56, 72, 0x123456789abcdef0ull, 88};
    static const uint64_t endCompact[6] = {68, 72, 76, 80, 84, 88}, endExtended[6] = {72, 80, 88, 96, 104, 112};   // the entries lie at 64
    for (int ext = 0; ext < 2; ext++) {
        const GfFileDir d{64, 32, ext, 1, 2, 2, 3, 6};
        for (int t = 0; t < 24; t++)
            if (gfDirEntryOfTile(d, t) != entryOfTile[t] || gfDirEntryAt(d, t / 6, t % 6) != entryOfTile[t]) return fail("rules", "a tile's entry", t);
        for (int k = 0; k < 6; k++)
            if (gfDirTileOfEntry(d, (uint64_t)k) != tileOfEntry[k]) return fail("rules", "an entry's tile", k);
        const uint64_t *want = ext ? posExtended : posCompact, *end = ext ? endExtended : endCompact;
        for (size_t n = 64; n <= end[5] + 1; n++) {
            uint8_t *block = (uint8_t *)calloc(n, 1);
            memcpy(block + 64, ext ? extended : compact, std::min<size_t>(n - 64, ext ? 48 : 24));
            for (int k = 0; k < 6; k++) {
                uint64_t pos = 99, posAligned = 99;
                const bool in = gfDirEntryPos(d, n, (uint64_t)k, &pos, GfLoadLe{block});
                const bool inAligned = gfDirEntryPos(d, n, (uint64_t)k, &posAligned, GfLoadAligned{block});
                if (in != (end[k] <= n) || inAligned != in || pos != (in ? want[k] : 0) || posAligned != pos) {
                    free(block);
                    return fail("rules", ext ? "an extended entry" : "a compact entry", (long)n * 8 + k);
                }
            }
            free(block);
        }
    }
    // {contentPos, bytes, P, behind} -> the first clause that fails
    static const struct { uint64_t contentPos, bytes, P, behind; GfPlace want; } places[] = {
        {96, 1004, 96, 12, GF_PLACE_IN_HEADER},   {96, 1004, 103, 12, GF_PLACE_IN_HEADER}, {96, 1004, 104, 12, GF_PLACE_OK},
        {96, 1004, 108, 12, GF_PLACE_OFF_GRID},   {96, 1004, 992, 12, GF_PLACE_OK},        {96, 1004, 993, 12, GF_PLACE_OFF_GRID},
        {96, 1003, 992, 12, GF_PLACE_HEAD_CUT},   {96, 1003, 992, 0, GF_PLACE_OK},         {96, 1000, 1000, 12, GF_PLACE_HEAD_CUT},
        {96, 1000, 1000, 0, GF_PLACE_OK},         {96, 1000, 1008, 12, GF_PLACE_BEHIND_END}, {96, 1000, 1008, 0, GF_PLACE_BEHIND_END},
        {96, 1000, 1004, 0, GF_PLACE_OFF_GRID},   {96, 100, 104, 0, GF_PLACE_BEHIND_END},  {96, 100, 96, 0, GF_PLACE_IN_HEADER}};
    for (size_t i = 0; i < sizeof(places) / sizeof(places[0]); i++)
        if (gfRecordPlace(places[i].contentPos, places[i].bytes, places[i].P, places[i].behind) != places[i].want) return fail("rules", "a place", (long)i);
    return 0;
}

int main(int argc, char **argv)
{
    if (rulesTable() != 0) return 1;
    uint64_t sum = 0;
    for (int a = 1; a < argc; a++) {
        FILE *fp = fopen(argv[a], "rb");
        if (!fp) return fail(argv[a], "cannot open", 0);
        std::vector<uint8_t> data;
        uint8_t buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof(buf), fp)) > 0;) data.insert(data.end(), buf, buf + n);
        fclose(fp);
        GfFileParsed p;
        if (gfFileParse(data.data(), data.size(), p) != GF_OK) return fail(argv[a], "the file does not open", 0);
        const gf_file_info &f = p.info;
        const GfFileDir d = gfFileDirOf(f);
        printf("%s %d.%02d grid %d %d %d %d checksums %d elems %d codecs %d content %llu dir %llu tiles", argv[a], f.version, f.subversion,
               f.grid.n_rows_grid, f.grid.n_cols_grid, f.grid.n_rows_tile, f.grid.n_cols_tile, f.checksum_enabled, f.n_elems, f.n_codecs,
               (unsigned long long)f.content_pos, (unsigned long long)f.tile_dir_pos);
        for (int t = 0; t < f.dir_n_rows * f.dir_n_cols; t++) {
            uint64_t pos;
            uint32_t size;
            if (gfFileLocate(d, data.data(), data.size(), t, &pos, &size) != GF_OK) return fail(argv[a], "a tile is not found", t);
            printf(" %llu", (unsigned long long)pos);
        }
        printf("\n");
        // every prefix, each in a block of its own length: open from the length that holds the header record and the directory's prefix
        const size_t enough = (size_t)(f.tile_dir_pos + GF_FILE_DIR_PREFIX);
        for (size_t n = 0; n <= data.size(); n++) {
            uint8_t *block = (uint8_t *)malloc(n ? n : 1);
            memcpy(block, data.data(), n);
            const gf_status s = openAndLocate(block, n, &sum);
            free(block);
            if ((s == GF_OK) != (n >= enough)) return fail(argv[a], "a prefix opens or fails at the wrong length", (long)n);
            if (s != GF_OK && s != (n < f.content_pos ? GF_ERR_BOUNDS : GF_ERR_FORMAT)) return fail(argv[a], "a prefix fails with the wrong status", (long)n);
        }
        // every byte of the header region, changed three ways: never GF_OK (with checksums, or a zero word without them, only the reserved
        // bytes of the file head could change unseen, and they lie in front of the region)
        uint8_t *block = (uint8_t *)malloc(data.size());
        for (size_t i = 16; i < f.content_pos; i++)
            for (const int x : {0x01, 0x80, 0xff}) {
                memcpy(block, data.data(), data.size());
                block[i] ^= (uint8_t)x;
                const gf_status s = openAndLocate(block, data.size(), &sum);
                if (f.checksum_enabled && s != GF_ERR_FORMAT && s != GF_ERR_BOUNDS)
                    return fail(argv[a], "a damaged header opens", (long)i);
            }
        // ... and every byte of the directory and of whatever lies behind it: the look-up never reads outside the image
        for (size_t i = (size_t)f.tile_dir_pos; i < data.size(); i++) {
            memcpy(block, data.data(), data.size());
            block[i] ^= 0xff;
            (void)openAndLocate(block, data.size(), &sum);
        }
        free(block);
    }
    printf("done %llu\n", (unsigned long long)(sum & 0xffff));
    return 0;
}
