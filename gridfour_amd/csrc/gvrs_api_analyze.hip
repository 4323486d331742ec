// gvrs_api_analyze.hip -- ICompressionDecoder.analyze of CodecHuffman and CodecCanonHuffman.

#include "gvrs_api_internal.h"

// ------------------------------------------------------------------ CodecHuffman.analyze

// ICompressionDecoder.analyze for a batch of CodecHuffman packings (compress/CodecHuffman.java:172-199): the packings are
// Huffman-decoded on the GPU, which returns per tile the predictor, the M32 byte count, the bits of the serialised tree and
// the 256-bin histogram of the M32 bytes; the sums of CodecStats.addToCounts / addCountsForM32 (compress/CodecStats.java:
// 100-141) are then accumulated here in tile order.  stats[p], p = 0..4 by predictor code (PredictorModelType ordinal),
// stats[5] = "All Predictors"; counts ADD to what stats already holds (clearAnalysisData = zero the array).  The pair
// counts behind CodecStats.getH2 (sA / sB) come from the same pass when the caller hands in tables for them.
// The packings of an analysis batch as a stage's inputs: blob | offsets | lengths (kept in *lengths for the host's part), and the
// statuses that come back.  Arguments as checked by the callers.
struct AnalyzeParts { int blob, offsets, lengths, status; };
static AnalyzeParts analyzeStage(HostStage &sg, size_t nTiles, const uint8_t *blob, const uint64_t *offsets, std::vector<uint32_t> *lengths,
                                 std::vector<int32_t> *st)
{
    lengths->resize(nTiles);
    st->resize(nTiles);
    for (size_t t = 0; t < nTiles; t++) (*lengths)[t] = (uint32_t)(offsets[t + 1] - offsets[t]);
    AnalyzeParts p;
    p.blob = sg.in(blob, (size_t)offsets[nTiles], 32), p.offsets = sg.in(offsets, (nTiles + 1) * 8);
    p.lengths = sg.in(lengths->data(), nTiles * 4), p.status = sg.out(st->data(), nTiles * 4);
    return p;
}

static gf_status analyzeBatch(gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob, const uint64_t *offsets,
                              gf_codec_stats *stats, int64_t *pairCounts, int32_t *status)
{
    if (!c || nRows < 1 || nCols < 1 || !blob || !offsets || !stats) return GF_ERR_ARG;
    if (!offsetsValid(offsets, nTiles)) return GF_ERR_ARG;    // a bad array must not become an out-of-bounds read
    GF_HIP(hipSetDevice(c->device));
    // staging: the packings | analysis records | a stand-in for the values, which an analysis does not write | the pair tables, zeroed
    const size_t pairWords = (size_t)GF_PAIR_TABLES * 65536;
    std::vector<uint32_t> lengths, rec(nTiles * GF_ANALYSIS_WORDS), pairs(pairCounts ? pairWords : 0);
    std::vector<int32_t> st;
    HostStage sg(c);
    const AnalyzeParts in = analyzeStage(sg, nTiles, blob, offsets, &lengths, &st);
    const int recP = sg.out(rec.data(), rec.size() * 4), valuesP = sg.local(16);
    const int pairsP = sg.add(pairCounts ? pairs.data() : nullptr, pairWords * 4, STAGE_OUT | STAGE_ZERO);
    gf_status s = sg.begin();
    if (s != GF_OK) return s;
    s = decodeBatchDev(KIND_HUFFMAN, c, c->stream, nRows, nCols, nTiles, sg.ptr<uint8_t>(in.blob), (size_t)offsets[nTiles],
                       sg.ptr<uint64_t>(in.offsets), 0, sg.ptr<uint32_t>(in.lengths), sg.ptr<int32_t>(valuesP), sg.ptr<int32_t>(in.status), 0,
                       sg.ptr<uint32_t>(recP), sg.ptr<uint32_t>(pairsP));
    if (s != GF_OK || (s = sg.end()) != GF_OK) return s;
    const double LOG2 = std::log(2.0);
    const int64_t nValues = (int64_t)nRows * nCols;
    for (size_t t = 0; t < nTiles; t++) {
        if (status) status[t] = st[t];
        if (st[t] != GF_OK) continue;                                   // analyze throws: nothing is counted
        const uint32_t *r = rec.data() + t * GF_ANALYSIS_WORDS;
        const uint32_t nM32 = r[1];
        int64_t observed = 0;
        double e = 0;
        if (nM32 > 0) {
            const double d = (double)nM32;
            for (int i = 0; i < 256; i++) {
                if (r[4 + i] > 0) {
                    observed++;
                    const double p = r[4 + i] / d;
                    e += p * std::log(p) / LOG2;
                }
            }
        }
        gf_codec_stats *two[2] = {&stats[r[0] <= 4 ? r[0] : 0], &stats[5]};
        for (gf_codec_stats *g : two) {
            g->n_tiles++;
            g->n_bytes += r[3];
            g->n_symbols += nValues;
            g->n_bits_overhead += r[2];
            if (nM32 > 0) {
                g->n_m32_counted++;
                g->sum_length_m32 += nM32;
                g->sum_observed_m32 += observed;
                g->sum_entropy_m32 -= e;
            }
        }
    }
    if (pairCounts) {
        // sB of the predictor's CodecStats and of "All Predictors" (CodecHuffman.java:186-196 feeds both)
        for (int m = 0; m < GF_PAIR_TABLES; m++)
            for (size_t i = 0; i < 65536; i++) {
                const int64_t n = pairs[(size_t)m * 65536 + i];
                pairCounts[(size_t)m * 65536 + i] += n;
                pairCounts[(size_t)5 * 65536 + i] += n;
            }
    }
    return GF_OK;
}

extern "C" {

gf_status gf_huffman_analyze_batch(gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob, const uint64_t *offsets,
                                   gf_codec_stats *stats, int32_t *status)
{
    GF_CTX_LOCK(c);
    return analyzeBatch(c, nRows, nCols, nTiles, blob, offsets, stats, nullptr, status);
}

gf_status gf_huffman_analyze_batch_h2(gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob,
                                      const uint64_t *offsets, gf_codec_stats *stats, int64_t *pairCounts, int32_t *status)
{
    GF_CTX_LOCK(c);
    if (!pairCounts) return GF_ERR_ARG;
    return analyzeBatch(c, nRows, nCols, nTiles, blob, offsets, stats, pairCounts, status);
}

// ------------------------------------------------------------------ CodecCanonHuffman.analyze

// ICompressionDecoder.analyze for a batch of CodecCanonHuffman packings (canonicalHuffman/CodecCanonHuffman.java:217-271):
// k_canon_decode<true> decodes the text of every packing on the GPU and k_canon_stats counts its symbols (CanonicalHuffman.
// countSymbols / getEntropy / getEscapeBitCountTotal); the host copies back a small record per tile and adds it to the
// CanonHuffmanStats sums in tile order -- the uniform form, the escape table and the record chosen by the predictor byte
// are decided here, from the packing, as analyze decides them.  stats[0..4] by PredictorModelType ordinal, stats[5] = "All
// Predictors"; stats and escape_counts are added to (clearAnalysisData = zero them).
gf_status gf_canon_analyze_batch(gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob, const uint64_t *offsets,
                                 gf_canon_stats *stats, int64_t *escapeCounts, int32_t *status)
{
    // (the arguments are checked before the context is touched)
    if (!c || nRows < 1 || nCols < 1 || !blob || !offsets || !stats || !escapeCounts) return GF_ERR_ARG;
    if (!offsetsValid(offsets, nTiles)) return GF_ERR_ARG;    // a bad array must not become an out-of-bounds read
    const size_t cells = (size_t)nRows * (size_t)nCols;
    if (cells >= (1ull << 28)) return GF_ERR_UNSUPPORTED;
    GF_CTX_LOCK(c);
    if (nTiles == 0) return GF_OK;
    GF_HIP(hipSetDevice(c->device));
    // staging: the packings | statistics records | the symbols of every tile
    std::vector<uint32_t> lengths, rec(nTiles * GF_CANON_STAT_WORDS);
    std::vector<int32_t> st;
    HostStage sg(c);
    const AnalyzeParts in = analyzeStage(sg, nTiles, blob, offsets, &lengths, &st);
    const int recP = sg.out(rec.data(), rec.size() * 4), valuesP = sg.local(nTiles * gf_canon_stats_stride((uint32_t)cells) * 4);
    gf_status s = sg.begin();
    if (s != GF_OK) return s;
    s = decodeBatchDev(KIND_CANON, c, c->stream, nRows, nCols, nTiles, sg.ptr<uint8_t>(in.blob), (size_t)offsets[nTiles],
                       sg.ptr<uint64_t>(in.offsets), 0, sg.ptr<uint32_t>(in.lengths), sg.ptr<int32_t>(valuesP), sg.ptr<int32_t>(in.status), 0,
                       sg.ptr<uint32_t>(recP));
    if (s != GF_OK || (s = sg.end()) != GF_OK) return s;
    const int64_t n = (int64_t)cells;
    auto add = [&](gf_canon_stats &g, int64_t nBytes, int64_t bitsInCodeTable, int64_t observed, double entropy) {
        g.n_tiles++;                                                    // CanonHuffmanStats.addToCounts
        g.n_bytes += nBytes;
        g.n_symbols += n;
        g.n_bits_overhead += bitsInCodeTable;
        g.n_text_counted++;                                             // addCountsForSymbols
        g.sum_length += n;
        g.sum_observed += observed;
        g.sum_entropy += entropy;
    };
    for (size_t t = 0; t < nTiles; t++) {
        int32_t tileStatus = st[t];
        if (tileStatus == GF_OK) {
            const uint8_t *pk = blob + offsets[t];
            const uint32_t predictor = pk[1];                           // packing[1] & 0xff
            if (predictor == 0 && lengths[t] == 6) {                    // the uniform form: n zeros, one symbol observed
                add(stats[0], 0, 0, 1, 0.0);
                add(stats[5], 0, 0, 1, 0.0);
            } else {
                const uint32_t *r = rec.data() + t * GF_CANON_STAT_WORDS;
                for (int k = 0; k < 6; k++) escapeCounts[k] += r[2 + k];   // before the predictor byte is used as an index
                if (predictor >= 6) {
                    tileStatus = GF_ERR_BOUNDS;                         // codecStats[predictor]: ArrayIndexOutOfBoundsException
                } else {
                    const int64_t escBits = (int64_t)(((uint64_t)r[9] << 32) | r[8]);
                    double entropy;
                    const uint64_t eb = ((uint64_t)r[11] << 32) | r[10];
                    std::memcpy(&entropy, &eb, 8);
                    add(stats[predictor], (int64_t)lengths[t] - 6, r[0], r[1], entropy);
                    add(stats[5], (int64_t)lengths[t] - 6, r[0], r[1], entropy);
                    stats[predictor].sum_escape_bits += escBits;        // (predictor byte 5: "All Predictors" twice)
                    stats[5].sum_escape_bits += escBits;
                }
            }
        }
        if (status) status[t] = tileStatus;
    }
    return GF_OK;
}

// CodecStats.getH2 (CodecStats.java:157-190) from one table of pair counts: sA[v] is the column sum of sB
double gf_codec_stats_h2(const int64_t *sB)
{
    if (!sB) return 0.0;
    std::vector<int64_t> sA(256, 0);
    int64_t k = 0;
    for (int p = 0; p < 256; p++)
        for (int v = 0; v < 256; v++) sA[v] += sB[p * 256 + v];
    for (int i = 0; i < 256; i++) k += sA[i];
    if (k == 0) return 0.0;
    double h2 = 0;
    for (int i = 0; i < 256; i++) {
        if (sA[i] > 0) {
            const double pI = (double)sA[i] / (double)k;
            int64_t n = 0;
            for (int j = i * 256; j < i * 256 + 256; j++) n += sB[j];
            double sumJ = 0;
            for (int j = i * 256; j < i * 256 + 256; j++)
                if (sB[j] > 0) {
                    const double pJ = (double)sB[j] / (double)n;
                    sumJ += pJ * std::log(pJ);
                }
            h2 += pI * sumJ;
        }
    }
    return -h2;
}

}  // extern "C"
