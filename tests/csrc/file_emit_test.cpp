// file_emit_test.cpp -- gvrs_file_emit.h alone, under the sanitizers: the reference's sample files taken apart (facts, metadata
// records' fields, tile records in file order) and assembled again, byte for byte; every image_cap from 0 to the need for the first
// two of them, each in a heap block of exactly image_cap bytes and once more in front of a guard region; an empty directory; the
// forced extended directory; metadata names and contents of length 0; and the CRC fold against the straight CRC for every pair of
// lengths 0 .. 2 chunks + 1, behind the host's CRC-32C itself against a bit-by-bit loop and the check value.
//   file_emit_test FILE...      prints "chunk N", one line per file and "done"; exit 0, or 1 with a message
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gridfour_amd/csrc/gvrs_file_emit.h"

static int fail(const char *path, const char *what, long at)
{
    printf("FAIL %s: %s at %ld\n", path, what, at);
    return 1;
}

static uint32_t le32(const std::vector<uint8_t> &d, uint64_t at) { return (uint32_t)d[at] | (uint32_t)d[at + 1] << 8 | (uint32_t)d[at + 2] << 16 | (uint32_t)d[at + 3] << 24; }

// the record at `at`: its size a multiple of 8 inside the image, its last word the CRC-32C of the bytes in front of it, or 0
static bool recordCrcBad(const std::vector<uint8_t> &d, uint64_t at, bool checksums)
{
    const uint32_t size = le32(d, at);
    if (size < 16 || (size & 7) != 0 || at + size > d.size()) return true;
    return le32(d, at + size - 4) != (checksums ? gfCrc32c(d.data() + at, size - 4) : 0u);
}

namespace {

// everything a sample says of itself that gf_file_assemble takes
struct Taken {
    GfFileParsed p;
    gf_file_facts facts;
    std::vector<gf_file_elem_facts> elemFacts;
    std::vector<std::string> labels, descriptions, units;
    std::vector<const char *> codecIds;
    std::vector<gf_file_metadata> metadata;
    std::vector<std::string> metaNames, metaDescriptions;
    std::vector<std::vector<uint8_t>> metaContents;
    std::vector<uint8_t> blob;
    std::vector<uint64_t> offsets;
    std::vector<int32_t> tileIndices;
};

static bool take(const std::vector<uint8_t> &d, Taken &t)
{
    if (gfFileParse(d.data(), d.size(), t.p) != GF_OK) return false;
    const gf_file_info &i = t.p.info;
    gf_file_facts &f = t.facts;
    memset(&f, 0, sizeof(f));
    f.grid = i.grid, f.n_elems = i.n_elems, f.n_codecs = i.n_codecs, f.elems = i.elems;
    f.checksum_enabled = i.checksum_enabled, f.raster_space = i.raster_space, f.coordinate_system = i.coordinate_system;
    f.x0 = i.x0, f.y0 = i.y0, f.x1 = i.x1, f.y1 = i.y1, f.cell_size_x = i.cell_size_x, f.cell_size_y = i.cell_size_y;
    memcpy(f.m2r, i.m2r, sizeof(f.m2r)), memcpy(f.r2m, i.r2m, sizeof(f.r2m));
    memcpy(f.uuid, d.data() + 24, 16);
    memcpy(&f.time_modified, d.data() + 40, 8);
    // what gf_file_info does not carry: the elements' continuous flags, ranges, labels, descriptions and units
    GfFileCursor c(d.data(), d.size(), i.content_pos, GF_FILE_SPEC_POS + 16 + 8 + 8 + 48 + 96 + 4);
    t.elemFacts.assign((size_t)i.n_elems, gf_file_elem_facts());
    t.labels.resize((size_t)i.n_elems), t.descriptions.resize((size_t)i.n_elems), t.units.resize((size_t)i.n_elems);
    for (int e = 0; e < i.n_elems; e++) {
        gf_file_elem_facts &x = t.elemFacts[(size_t)e];
        const int code = c.u8();
        x.continuous = c.u8();
        c.skip(6);
        (void)c.utf();
        c.alignTo4();
        x.has_range = 1;
        if (code == 0) x.range.min_i = c.i32(), x.range.max_i = c.i32(), c.skip(4);
        else if (code == 1) x.range.min_f = c.f32(), x.range.max_f = c.f32(), c.skip(12), x.range.min_i = c.i32(), x.range.max_i = c.i32(), c.skip(4);
        else if (code == 2) x.range.min_f = c.f32(), x.range.max_f = c.f32(), c.skip(4);
        else x.range.min_i = c.i16(), x.range.max_i = c.i16(), c.skip(2);
        t.labels[(size_t)e] = c.utf(), t.descriptions[(size_t)e] = c.utf(), t.units[(size_t)e] = c.utf();
        c.alignTo4();
    }
    if (c.status != GF_OK) return false;
    for (int e = 0; e < i.n_elems; e++) {
        gf_file_elem_facts &x = t.elemFacts[(size_t)e];
        x.name = t.p.elemNames[(size_t)e].c_str(), x.label = t.labels[(size_t)e].c_str();
        x.description = t.descriptions[(size_t)e].c_str(), x.unit = t.units[(size_t)e].c_str();
    }
    f.elem_facts = t.elemFacts.data();
    for (const std::string &s : t.p.codecIds) t.codecIds.push_back(s.c_str());
    f.codec_ids = t.codecIds.data();
    f.product_label = t.p.productLabel.c_str();
    // the metadata records, through the metadata directory (in order of position)
    if (i.metadata_dir_pos) {
        GfFileCursor m(d.data(), d.size(), d.size(), i.metadata_dir_pos);
        const int32_t n = m.i32();
        t.metadata.assign((size_t)n, gf_file_metadata());
        t.metaNames.resize((size_t)n), t.metaDescriptions.resize((size_t)n), t.metaContents.resize((size_t)n);
        for (int32_t k = 0; k < n; k++) {
            const uint64_t pos = m.u64();
            (void)m.utf();
            m.skip(5);
            GfFileCursor r(d.data(), d.size(), d.size(), pos);
            t.metaNames[(size_t)k] = r.utf();
            t.metadata[(size_t)k].record_id = r.i32();
            t.metadata[(size_t)k].type = r.u8();
            r.skip(3);
            const int32_t nb = r.i32();
            if (!r.need((uint64_t)nb)) return false;
            t.metaContents[(size_t)k].assign(d.data() + r.pos, d.data() + r.pos + nb);
            r.skip((uint64_t)nb);
            t.metaDescriptions[(size_t)k] = r.utf();
            if (r.status != GF_OK) return false;
        }
        if (m.status != GF_OK) return false;
        for (int32_t k = 0; k < n; k++) {
            gf_file_metadata &x = t.metadata[(size_t)k];
            x.name = t.metaNames[(size_t)k].c_str(), x.description = t.metaDescriptions[(size_t)k].c_str();
            x.content = t.metaContents[(size_t)k].data(), x.content_bytes = t.metaContents[(size_t)k].size();
        }
    }
    // the tile records in file order
    const GfFileDir dir = gfFileDirOf(i);
    const int32_t nTiles = dir.nColsOfTiles * ((i.grid.n_rows_grid + i.grid.n_rows_tile - 1) / i.grid.n_rows_tile);
    std::vector<std::pair<uint64_t, int32_t>> at;
    for (int32_t k = 0; k < nTiles; k++) {
        uint64_t pos;
        uint32_t size;
        if (gfFileLocate(dir, d.data(), d.size(), k, &pos, &size) != GF_OK) return false;
        if (pos) at.push_back(std::make_pair(pos, k));
    }
    std::sort(at.begin(), at.end());
    t.offsets.assign(1, 0);
    for (const auto &a : at) {
        const uint32_t size = (uint32_t)d[a.first - 8] | (uint32_t)d[a.first - 7] << 8 | (uint32_t)d[a.first - 6] << 16 | (uint32_t)d[a.first - 5] << 24;
        t.blob.insert(t.blob.end(), d.begin() + (long)(a.first - 8), d.begin() + (long)(a.first - 8 + size));
        t.offsets.push_back(t.blob.size());
        t.tileIndices.push_back(a.second);
    }
    return true;
}

static gf_status assemble(const Taken &t, int flags, size_t nRecords, uint8_t *image, size_t cap, uint64_t *bytes)
{
    return gfFileAssemble(t.facts, t.metadata.data(), (int)t.metadata.size(), flags, t.blob.data(), t.offsets.data(), t.tileIndices.data(), nRecords, image,
                          cap, bytes);
}

}  // namespace

// the shared gfCrc32c (eight bytes a step) against a bit-by-bit loop: every length 0 .. 40 at every start offset 0 .. 7 of a buffer
// (head, 8-byte body and tail), and the check value of the nine digits
static int crcStraight()
{
    uint8_t bytes[48];
    uint32_t x = 2463534242u;
    for (uint8_t &b : bytes) x = x * 1664525u + 1013904223u, b = (uint8_t)(x >> 24);
    for (size_t at = 0; at < 8; at++)
        for (size_t n = 0; n <= 40; n++) {
            uint32_t crc = 0xffffffffu;
            for (size_t i = 0; i < n; i++) {
                crc ^= bytes[at + i];
                for (int k = 0; k < 8; k++) crc = (crc >> 1) ^ ((crc & 1u) ? 0x82F63B78u : 0u);
            }
            if (gfCrc32c(bytes + at, n) != ~crc) return fail("crc", "gfCrc32c differs from the bit-by-bit loop", (long)(at * 1000 + n));
        }
    if (gfCrc32c((const uint8_t *)"123456789", 9) != 0xE3069283u) return fail("crc", "gfCrc32c misses the check value", 0);
    return 0;
}

static int crcFold()
{
    const size_t top = 2 * GF_FILE_CRC_CHUNK + 1;
    std::vector<uint8_t> bytes(2 * top);
    uint32_t x = 12345u;
    for (uint8_t &b : bytes) x = x * 1664525u + 1013904223u, b = (uint8_t)(x >> 24);
    std::vector<uint32_t> xpow(top + 1), whole(2 * top + 1);
    for (size_t n = 0; n <= top; n++) xpow[n] = gfCrcXpow8n(n);
    for (size_t n = 0; n <= 2 * top; n++) whole[n] = gfCrc32c(bytes.data(), n);              // the straight CRC of every prefix
    for (size_t a = 0; a <= top; a++) {
        uint32_t run = 0xffffffffu;                                                              // crc of bytes[a, a + b), byte by byte
        for (size_t b = 0; b <= top; b++) {
            if (gfCrc32cFold(whole[a], ~run, xpow[b]) != whole[a + b]) return fail("crc", "the fold differs from the straight CRC", (long)(a * 100000 + b));
            if (b < top) {
                run ^= bytes[a + b];
                for (int k = 0; k < 8; k++) run = (run >> 1) ^ ((run & 1u) ? 0x82F63B78u : 0u);
            }
        }
    }
    for (const size_t n : {(size_t)0, (size_t)1, (size_t)GF_FILE_CRC_CHUNK - 1, (size_t)GF_FILE_CRC_CHUNK, (size_t)GF_FILE_CRC_CHUNK + 1, 2 * top})
        if (gfFileCrc32cChunked(bytes.data(), n) != whole[n] || gfCrc32cCombine(whole[n / 3], gfCrc32c(bytes.data() + n / 3, n - n / 3), n - n / 3) != whole[n])
            return fail("crc", "the chunked CRC differs", (long)n);
    return 0;
}

int main(int argc, char **argv)
{
    printf("chunk %u\n", GF_FILE_CRC_CHUNK);
    for (int a = 1; a < argc; a++) {
        FILE *fp = fopen(argv[a], "rb");
        if (!fp) return fail(argv[a], "cannot open", 0);
        std::vector<uint8_t> data;
        uint8_t buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof(buf), fp)) > 0;) data.insert(data.end(), buf, buf + n);
        fclose(fp);
        Taken t;
        if (!take(data, t)) return fail(argv[a], "the sample cannot be taken apart", 0);
        const size_t nRec = t.tileIndices.size();
        uint64_t need = 0;
        if (assemble(t, 0, nRec, nullptr, 0, &need) != GF_ERR_CAPACITY || need != data.size()) return fail(argv[a], "the need is not the file's size", (long)need);
        std::vector<uint8_t> image(need);
        if (assemble(t, 0, nRec, image.data(), need, &need) != GF_OK) return fail(argv[a], "the image is not assembled", 0);
        for (size_t k = 0; k < need; k++)
            if (image[k] != data[k]) return fail(argv[a], "the image differs from the file", (long)k);
        printf("%s same %llu records %zu metadata %zu\n", argv[a], (unsigned long long)need, nRec, t.metadata.size());
        if (a <= 2) {
            // every capacity: below the need nothing is written (a block of exactly cap bytes; and a guard region behind a larger one)
            const size_t guard = 64;
            for (size_t cap = 0; cap <= need; cap++) {
                uint8_t *exact = (uint8_t *)malloc(cap ? cap : 1), *wide = (uint8_t *)malloc(need + guard);
                memset(wide, 0xCD, need + guard);
                uint64_t got = 0, got2 = 0;
                const gf_status s = assemble(t, 0, nRec, exact, cap, &got), s2 = assemble(t, 0, nRec, wide, cap, &got2);
                bool ok = s == (cap < need ? GF_ERR_CAPACITY : GF_OK) && s2 == s && got == need && got2 == need;
                for (size_t k = cap < need ? 0 : need; ok && k < need + guard; k++) ok = wide[k] == 0xCD;
                if (ok && cap == need) ok = memcmp(exact, data.data(), need) == 0 && memcmp(wide, data.data(), need) == 0;
                free(exact), free(wide);
                if (!ok) return fail(argv[a], "a capacity is handled wrongly", (long)cap);
            }
        }
        // no records: the empty directory of 40 bytes, and the image opens with every tile absent
        uint64_t bytes0 = 0;
        (void)assemble(t, 0, 0, nullptr, 0, &bytes0);
        std::vector<uint8_t> empty(bytes0);
        if (assemble(t, 0, 0, empty.data(), bytes0, &bytes0) != GF_OK) return fail(argv[a], "the image without records is not assembled", 0);
        GfFileParsed q;
        if (gfFileParse(empty.data(), empty.size(), q) != GF_OK) return fail(argv[a], "the image without records does not open", 0);
        if (q.info.dir_n_rows || q.info.dir_n_cols || q.info.dir_row0 || q.info.dir_col0 || q.info.tile_dir_pos + 32 != bytes0 ||
            empty[q.info.tile_dir_pos - 8] != 40)
            return fail(argv[a], "the empty directory is not 40 bytes of zeros", (long)bytes0);
        // the forced extended directory: every tile is found where the compact one names it
        uint64_t bytesX = 0;
        (void)assemble(t, GF_FILE_DIR_EXTENDED, nRec, nullptr, 0, &bytesX);
        std::vector<uint8_t> ext(bytesX);
        if (assemble(t, GF_FILE_DIR_EXTENDED, nRec, ext.data(), bytesX, &bytesX) != GF_OK) return fail(argv[a], "the extended image is not assembled", 0);
        if (gfFileParse(ext.data(), ext.size(), q) != GF_OK || !q.info.dir_extended) return fail(argv[a], "the extended image does not open", 0);
        const uint64_t dirAt = q.info.tile_dir_pos - 8, dirSize = gfFileTileDirSize((uint64_t)q.info.dir_n_rows * (uint64_t)q.info.dir_n_cols, true);
        if (dirAt + dirSize != bytesX || recordCrcBad(ext, dirAt, t.facts.checksum_enabled != 0)) return fail(argv[a], "the extended directory's record is wrong", (long)dirAt);
        const GfFileDir dc = gfFileDirOf(t.p.info), dx = gfFileDirOf(q.info);
        for (size_t r = 0; r < nRec; r++) {
            uint64_t pc, px;
            uint32_t sc, sx;
            if (gfFileLocate(dc, data.data(), data.size(), t.tileIndices[r], &pc, &sc) != GF_OK ||
                gfFileLocate(dx, ext.data(), ext.size(), t.tileIndices[r], &px, &sx) != GF_OK || pc != px || sc != sx)
                return fail(argv[a], "the extended directory names another place", (long)r);
        }
        // metadata with names, contents and descriptions of length 0
        const uint8_t one = 7;
        const gf_file_metadata zero[3] = {{"", "", nullptr, 0, 1, 0}, {"a", nullptr, &one, 0, -5, 3}, {nullptr, "d", &one, 1, 0, 6}};
        uint64_t bytesM = 0;
        (void)gfFileAssemble(t.facts, zero, 3, 0, t.blob.data(), t.offsets.data(), t.tileIndices.data(), nRec, nullptr, 0, &bytesM);
        std::vector<uint8_t> meta(bytesM);
        if (gfFileAssemble(t.facts, zero, 3, 0, t.blob.data(), t.offsets.data(), t.tileIndices.data(), nRec, meta.data(), bytesM, &bytesM) != GF_OK)
            return fail(argv[a], "the image with empty metadata is not assembled", 0);
        if (gfFileParse(meta.data(), meta.size(), q) != GF_OK || q.info.metadata_dir_pos == 0) return fail(argv[a], "the image with empty metadata does not open", 0);
        GfFileCursor m(meta.data(), meta.size(), meta.size(), q.info.metadata_dir_pos);
        if (m.i32() != 3 || recordCrcBad(meta, q.info.metadata_dir_pos - 8, t.facts.checksum_enabled != 0)) return fail(argv[a], "the metadata directory is wrong", 0);
        uint64_t expect = q.info.content_pos + 8;
        for (int k = 0; k < 3; k++) {
            const uint64_t pos = m.u64();
            const std::string name = m.utf();
            const int32_t id = m.i32();
            const int type = m.u8();
            if (pos != expect || name != (zero[k].name ? zero[k].name : "") || id != zero[k].record_id || type != zero[k].type)
                return fail(argv[a], "a metadata directory entry is wrong", k);
            if (recordCrcBad(meta, pos - 8, t.facts.checksum_enabled != 0)) return fail(argv[a], "a metadata record's frame is wrong", k);
            GfFileCursor r(meta.data(), meta.size(), meta.size(), pos);
            if (r.utf() != name || r.i32() != id || r.u8() != type) return fail(argv[a], "a metadata record is wrong", k);
            r.skip(3);
            if (r.i32() != (int32_t)zero[k].content_bytes) return fail(argv[a], "a metadata record's content is wrong", k);
            r.skip(zero[k].content_bytes);
            if (r.utf() != (zero[k].description ? zero[k].description : "") || r.status != GF_OK) return fail(argv[a], "a metadata record's description is wrong", k);
            expect = pos + le32(meta, pos - 8);
        }
        const GfFileDir dm = gfFileDirOf(q.info);
        uint64_t first = ~0ull;
        for (size_t r = 0; r < nRec; r++) {
            uint64_t pos;
            uint32_t size;
            if (gfFileLocate(dm, meta.data(), meta.size(), t.tileIndices[r], &pos, &size) != GF_OK || pos == 0) return fail(argv[a], "a tile is lost", (long)r);
            first = std::min(first, pos);
        }
        if (nRec && first != expect) return fail(argv[a], "the records do not follow the metadata records end to end", (long)expect);
    }
    if (crcStraight() || crcFold()) return 1;
    printf("done\n");
    return 0;
}
