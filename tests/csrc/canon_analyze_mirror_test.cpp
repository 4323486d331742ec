// Exercises CodecCanonHuffmanHip's analysis in the C++ host mirror (gridfour_amd/host/gvrs_hip_codec.hpp).  Without a GPU:
// construction fails loudly, and the analysis entry point rejects bad arguments.  With a GPU: argv[1] names a file of
// packings ("<nRows> <nCols> <nTiles>" then per tile "<length> <hex bytes>"); the program analyzes them one by one and
// as a batch and prints the sums, the escape table and the report for the Python test to compare.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "../../gridfour_amd/host/gvrs_hip_codec.hpp"

static void print(const gridfour::CodecCanonHuffmanHip &c, const char *tag)
{
    const gf_canon_stats *s = c.analysisData();
    for (int k = 0; k < 6; k++)
        std::printf("%s %d %ld %ld %ld %ld %ld %ld %ld %.17g %ld\n", tag, k, (long)s[k].n_tiles, (long)s[k].n_bytes, (long)s[k].n_symbols,
                    (long)s[k].n_bits_overhead, (long)s[k].n_text_counted, (long)s[k].sum_length, (long)s[k].sum_observed,
                    s[k].sum_entropy, (long)s[k].sum_escape_bits);
    std::printf("%s escapes", tag);
    for (int i = 0; i < 6; i++) std::printf(" %ld", (long)c.escapeCounts()[i]);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    {
        gf_canon_stats stats[6] = {};
        int64_t esc[6] = {};
        const uint8_t blob[16] = {};
        const uint64_t bad[3] = {0, 10, 5};
        if (gf_canon_analyze_batch(nullptr, 4, 4, 2, blob, bad, stats, esc, nullptr) != GF_ERR_ARG) { std::puts("null context accepted"); return 6; }
    }
    try {
        gridfour::CodecCanonHuffmanHip codec(0);
        if (argc < 2) { std::puts("usage: canon_analyze_mirror_test <packings>"); return 2; }
        std::ifstream in(argv[1]);
        int nRows = 0, nCols = 0;
        size_t nTiles = 0;
        in >> nRows >> nCols >> nTiles;
        std::vector<std::vector<uint8_t>> packs(nTiles);
        for (auto &p : packs) {
            size_t len = 0;
            in >> len;
            p.resize(len);
            for (auto &b : p) { unsigned x; in >> std::hex >> x >> std::dec; b = (uint8_t)x; }
        }
        codec.clearAnalysisData();
        std::vector<int32_t> single;
        for (const auto &p : packs) {
            int32_t st = GF_OK;
            try { codec.analyze(nRows, nCols, p); } catch (const gridfour::IOException &) { st = -1; }
            single.push_back(st);
        }
        print(codec, "single");
        std::printf("single status");
        for (int32_t s : single) std::printf(" %d", s);
        std::printf("\n");
        codec.clearAnalysisData();
        std::vector<uint8_t> blob;
        std::vector<uint64_t> offsets{0};
        for (const auto &p : packs) { blob.insert(blob.end(), p.begin(), p.end()); offsets.push_back(blob.size()); }
        blob.resize(blob.size() + 16);
        const std::vector<int32_t> st = codec.analyzeBatch(nRows, nCols, nTiles, blob.data(), offsets.data());
        print(codec, "batch");
        std::printf("batch status");
        for (int32_t s : st) std::printf(" %d", s);
        std::printf("\n");
        codec.reportAnalysisData(stdout, (int)nTiles);
        codec.clearAnalysisData();
        codec.reportAnalysisData(stdout, (int)nTiles);
        return 0;
    } catch (const std::runtime_error &e) {
        std::printf("no-device: %s\n", e.what());
        return 10;
    }
}
