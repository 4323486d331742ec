// gvrs_api_deflate.hip -- CodecDeflate (predictor + M32 on the GPU, Deflate on the host; decoded on the device), CodecMaster over
// a codec list and the tile payloads.

#include "gvrs_api_internal.h"

// ---- Deflate-carrying containers decoded on the device: walk the packings, inflate (gvrs_inflate.hip), decode ----------
// The scratch (inflated bytes, stream descriptors, per-stream results) is bounded: batches go through it in chunks of tiles,
// one after the other in stream order.

gf_status deflateDecodeDev(gf_context *c, hipStream_t st, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob, size_t blobBytes,
                           const uint64_t *dOffsets, size_t slotStride, const uint32_t *dLengths, int32_t *dValues, int32_t *dStatus)
{
    const size_t cells = (size_t)nRows * (size_t)nCols;
    if (cells >= (1ull << 28)) return GF_ERR_UNSUPPORTED;
    const size_t rawStride = roundUp(10 + 6 * cells, 16);                 // an M32 stream has at most six bytes per cell
    const size_t chunk = std::max<size_t>(1, std::min(nTiles, INFLATE_SCRATCH_BYTES / rawStride));
    gf_status s;
    if ((s = c->dInflOut.ensure(chunk * rawStride + 64)) != GF_OK) return s;
    if ((s = c->dInflate.ensure(chunk * sizeof(GfInflateStream) + 64)) != GF_OK) return s;
    Carve k;
    size_t at[5];                                                        // per stream: produced, M32 length, status of inflate, walk, decode
    for (size_t &x : at) x = k.add(chunk * 4);
    if ((s = c->dInflMeta.ensure(k, 256)) != GF_OK) return s;
    uint8_t *raw = (uint8_t *)c->dInflOut.p;
    GfInflateStream *desc = (GfInflateStream *)c->dInflate.p;
    uint32_t *produced = c->dInflMeta.at<uint32_t>(at[0]), *rawLengths = c->dInflMeta.at<uint32_t>(at[1]);
    int32_t *inflStatus = c->dInflMeta.at<int32_t>(at[2]), *pre = c->dInflMeta.at<int32_t>(at[3]), *decStatus = c->dInflMeta.at<int32_t>(at[4]);
    for (size_t t0 = 0; t0 < nTiles; t0 += chunk) {
        const size_t n = std::min(chunk, nTiles - t0);
        GF_HIP(gf_launch_deflate_streams(dBlob, blobBytes, dOffsets, slotStride, dLengths, t0, n, (uint32_t)cells, raw, rawStride, desc, pre, st));
        GfInflateArgs a{};
        a.inBase = dBlob;
        a.outBase = raw;
        a.streams = desc;
        a.produced = produced;
        a.status = inflStatus;
        a.nStreams = n;
        a.window = gf_inflate_window((uint32_t)std::min<size_t>(6 * cells, 32768));
        GF_HIP(gf_launch_inflate(a, st));
        GF_HIP(gf_launch_deflate_lengths(n, desc, produced, inflStatus, pre, rawLengths, raw, st));
        s = decodeBatchDev(KIND_RAW_M32, c, st, nRows, nCols, n, raw, chunk * rawStride + 32, nullptr, rawStride, rawLengths,
                           dValues + t0 * cells, decStatus, 0);
        if (s != GF_OK) return s;
        GF_HIP(gf_launch_merge_status(n, pre, decStatus, dStatus + t0, st));
    }
    return GF_OK;
}

// CodecDeflate.encode :157-199 + compress :201-228 for a batch in host memory: the candidate M32 streams come from the GPU,
// java.util.zip.Deflater(6) is the host's zlib, the strictly shortest packing wins (earlier predictor on ties).
//
// The cost is zlib's: three candidate streams per tile at level 6 (tools/codec_master_rate.py: 60 MB/s of M32 bytes per core,
// 0.9 ms per 120x150 tile and core).  What can be done around it is done (round 3): the batch goes through in chunks, the GPU
// stage of chunk k + 1 (upload, k_m32_streams, download) overlapping the host threads' zlib of chunk k; a candidate is given
// up the moment its stream is longer than the shortest packing known for the tile -- the predictors' candidates among each
// other (Triangle first: it is the shortest on terrain, the ties of :195 are kept by comparing against the right side), and
// under gf_codec_master_encode_batch_i32 the packings of the list's other codecs (notLongerThan): a candidate that cannot win
// needs no bytes.  Results are byte-identical to running every stream to its end.
static gf_status deflateEncodeBatchHost(gf_context *c, int codecIndex, int nRows, int nCols, size_t nTiles, const int32_t *values,
                                        const uint32_t *notLongerThan,      // per tile or null: packings longer than this are of no use
                                        std::vector<std::vector<uint8_t>> &packs, std::vector<uint8_t> &chosen, std::vector<int32_t> &st)
{
    GF_HIP(hipSetDevice(c->device));
    const size_t cells = (size_t)nRows * (size_t)nCols;
    const size_t sub = gf_m32_default_stride(nRows, nCols), maxSub = gf_m32_max_stream(nRows, nCols);
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(nTiles, (size_t)(64u << 20) / (cells * 4)));
    gf_status s;
    if ((s = c->dValues.ensure(chunk * cells * 4 + 16)) != GF_OK) return s;
    if ((s = c->dM32.ensure(chunk * 3 * sub + 16)) != GF_OK) return s;
    if ((s = c->dM32Len.ensure(chunk * 12 + 16)) != GF_OK) return s;
    if ((s = c->dM32Models.ensure(chunk * 3 + 16)) != GF_OK) return s;
    if ((s = c->dSeeds.ensure(chunk * 4 + 16)) != GF_OK) return s;
    if ((s = c->dStatus.ensure(chunk * 4 + 16)) != GF_OK) return s;
    packs.assign(nTiles, {});
    chosen.assign(nTiles, 0);
    st.assign(nTiles, GF_OK);
    struct Stage {                                                       // what a chunk brings back from the GPU
        std::unique_ptr<uint8_t[]> streams;
        std::vector<uint8_t> models;
        std::vector<uint32_t> lens, seeds;
        std::vector<std::vector<uint8_t>> big;                           // tiles whose streams did not fit the default sub-slot
        size_t t0 = 0, n = 0;
    } stage[2];
    for (Stage &g : stage) g.streams.reset(new uint8_t[chunk * 3 * sub]);
    auto gpuStage = [&](Stage &g, size_t t0, size_t n) -> gf_status {
        g.t0 = t0;
        g.n = n;
        g.models.resize(n * 3);
        g.lens.resize(n * 3);
        g.seeds.resize(n);
        g.big.assign(n, {});
        GF_HIP(hipMemcpyAsync(c->dValues.p, values + t0 * cells, n * cells * 4, hipMemcpyHostToDevice, c->stream));
        gf_status r = gf_m32_encode_batch_i32_dev(c, c->stream, nRows, nCols, n, (const int32_t *)c->dValues.p, (uint8_t *)c->dM32.p, sub,
                                                  (uint32_t *)c->dM32Len.p, (uint8_t *)c->dM32Models.p, (uint32_t *)c->dSeeds.p,
                                                  (int32_t *)c->dStatus.p);
        if (r != GF_OK) return r;
        GF_HIP(hipMemcpyAsync(g.streams.get(), c->dM32.p, n * 3 * sub, hipMemcpyDeviceToHost, c->stream));
        GF_HIP(hipMemcpyAsync(g.lens.data(), c->dM32Len.p, n * 12, hipMemcpyDeviceToHost, c->stream));
        GF_HIP(hipMemcpyAsync(g.models.data(), c->dM32Models.p, n * 3, hipMemcpyDeviceToHost, c->stream));
        GF_HIP(hipMemcpyAsync(g.seeds.data(), c->dSeeds.p, n * 4, hipMemcpyDeviceToHost, c->stream));
        GF_HIP(hipMemcpyAsync(st.data() + t0, c->dStatus.p, n * 4, hipMemcpyDeviceToHost, c->stream));
        GF_HIP(hipStreamSynchronize(c->stream));
        // tiles with a stream longer than the default sub-slot: once more, one at a time, into worst-case slots
        for (size_t i = 0; i < n; i++) {
            if (st[t0 + i] != GF_OVERFLOW) continue;
            DevBuf slot, meta;
            if ((r = slot.ensure(3 * maxSub)) != GF_OK) return r;
            if ((r = meta.ensure(64)) != GF_OK) { slot.release(); return r; }
            uint8_t *m = (uint8_t *)meta.p;
            r = gf_m32_encode_batch_i32_dev(c, c->stream, nRows, nCols, 1, (const int32_t *)c->dValues.p + i * cells, (uint8_t *)slot.p,
                                            maxSub, (uint32_t *)m, m + 16, (uint32_t *)(m + 32), (int32_t *)(m + 48));
            g.big[i].resize(3 * maxSub);
            hipError_t e1 = hipSuccess, e2 = hipSuccess, e3 = hipSuccess;
            if (r == GF_OK) {
                e1 = hipMemcpyAsync(g.big[i].data(), slot.p, 3 * maxSub, hipMemcpyDeviceToHost, c->stream);
                e2 = hipMemcpyAsync(&st[t0 + i], m + 48, 4, hipMemcpyDeviceToHost, c->stream);
                e3 = hipStreamSynchronize(c->stream);
            }
            slot.release();
            meta.release();
            if (r != GF_OK) return r;
            if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return hipFail(e1 != hipSuccess ? e1 : e2 != hipSuccess ? e2 : e3, "m32 overflow tile");
        }
        return GF_OK;
    };
    auto zlibStage = [&](const Stage &g) {
        parallelFor(g.n, [&](size_t i) {
            const size_t t = g.t0 + i;
            if (st[t] != GF_OK) return;
            const bool isBig = !g.big[i].empty();
            const size_t stride = isBig ? maxSub : sub;
            const uint8_t *base = isBig ? g.big[i].data() : g.streams.get() + i * 3 * sub;
            // packing length of the candidate kept so far per predictor slot (0: none); the winner is the FIRST shortest in the
            // order Differencing, Linear, Triangle (:195: a later one must be strictly shorter)
            size_t have[3] = {0, 0, 0};
            std::vector<uint8_t> z[3];
            static const int order[3] = {2, 0, 1};                           // Triangle first, then the reference's order
            for (int oi = 0; oi < 3; oi++) {
                const int p = order[oi];
                const uint32_t n = g.lens[i * 3 + p];
                const int model = g.models[i * 3 + p];
                if (model == 0 || n == 0) continue;                          // mCodeLength > 0 (:189)
                // longest packing this candidate is still of use with: against an EARLIER slot it must be strictly shorter,
                // against a LATER one no longer
                size_t cap = notLongerThan ? (size_t)notLongerThan[t] : ~(size_t)0;
                for (int q = 0; q < 3; q++)
                    if (have[q]) cap = std::min(cap, q < p ? have[q] - 1 : have[q]);
                if (cap < 11) continue;
                const size_t limit = std::min<size_t>(cap - 10, (size_t)n + 118);   // Deflater wrote into byte[nM32 + 128] from offset 10 (:204-205)
                if (!zDeflateUpTo(base + p * stride, n, 6, limit, z[p])) {
                    // given up: longer than the limit.  The reference's buffer cuts a stream at nM32 + 118 bytes; a candidate that
                    // long is kept at that length there -- run it to the end where that cut is the reason
                    if (limit == (size_t)n + 118 && zDeflate(base + p * stride, n, 6, z[p])) z[p].resize(limit);
                    else continue;
                }
                if (z[p].empty()) continue;
                have[p] = z[p].size() + 10;
            }
            int win = -1;
            for (int p = 0; p < 3; p++)
                if (have[p] && (win < 0 || have[p] < have[win])) win = p;
            if (win < 0) { st[t] = GF_DECLINED; return; }
            std::vector<uint8_t> &pk = packs[t];
            pk.resize(have[win]);
            pk[0] = (uint8_t)codecIndex;
            pk[1] = g.models[i * 3 + win];
            putLE32(&pk[2], g.seeds[i]);
            putLE32(&pk[6], g.lens[i * 3 + win]);
            memcpy(&pk[10], z[win].data(), z[win].size());
            chosen[t] = g.models[i * 3 + win];
        });
    };
    // chunk k's zlib runs on the host's threads while this thread drives the GPU stage of chunk k + 1
    // (joined by a guard: an exception on this thread -- a vector that cannot grow -- must not meet a joinable std::thread, which
    // would end the process; one on the worker thread is caught there and becomes a status)
    struct Joined {
        std::thread t;
        ~Joined() { if (t.joinable()) t.join(); }
    } worker;
    std::atomic<int> workerStatus{GF_OK};
    gf_status result = GF_OK;
    int cur = 0;
    try {
        for (size_t t0 = 0; t0 < nTiles && result == GF_OK; t0 += chunk) {
            const size_t n = std::min(chunk, nTiles - t0);
            result = gpuStage(stage[cur], t0, n);
            if (worker.t.joinable()) worker.t.join();
            if (result != GF_OK) break;
            Stage *g = &stage[cur];
            worker.t = std::thread([&, g]() {
                try {
                    zlibStage(*g);
                } catch (const std::bad_alloc &) {
                    workerStatus = GF_ERR_HIP;
                }
            });
            cur ^= 1;
        }
    } catch (const std::bad_alloc &) {
        result = GF_ERR_HIP;
    }
    if (worker.t.joinable()) worker.t.join();
    if (result == GF_OK && workerStatus != GF_OK) {
        g_lastError = "out of host memory in the Deflate stage";
        result = (gf_status)workerStatus.load();
    }
    return result;
}

// gvrs/CodecMaster.java:195-203: dispatch on packing[0]
// CodecMaster.decode (gvrs/CodecMaster.java:195-203) for packings anywhere inside `blob`: packing t is lens[t] bytes at
// blob + starts[t]; tiles with skip[t] != 0 are left alone (raw elements, records that failed their checks).  The packings are
// sorted by the codec their first byte names and every codec's share goes through its batch decoder in the scattered form
// (decodeBatchHostG): nothing is copied on the host but the packings themselves, into the pinned staging buffers, and the
// decoded tiles from there to their place.  (Round 3 built a fresh blob per codec with vector::insert per tile, decoded into a
// temporary array and copied every tile back, single-threaded: 2.9 GB/s on top of a 40 GB/s decoder.)
gf_status codecMasterDecodeScattered(gf_context *c, const int *codecs, int nCodecs, int nRows, int nCols, size_t nTiles,
                                     const uint8_t *blob, const uint64_t *starts, const uint32_t *lens, const uint8_t *skip,
                                     int32_t *values, int32_t *st)
{
    const size_t cells = (size_t)nRows * (size_t)nCols;
    std::vector<uint32_t> count(256, 0);
    for (size_t t = 0; t < nTiles; t++) {
        if (skip && skip[t]) continue;
        const int k = lens[t] ? (int)blob[starts[t]] : -1;
        if (k < 0 || k >= nCodecs || codecs[k] == GF_CODEC_NONE) { st[t] = GF_ERR_FORMAT; continue; }   // no such codec in the list
        count[k]++;
    }
    for (int k = 0; k < nCodecs && k < 256; k++) {
        if (!count[k]) continue;
        std::vector<uint64_t> ks(count[k]);
        std::vector<uint32_t> kl(count[k]), kd(count[k]);
        size_t i = 0;
        for (size_t t = 0; t < nTiles; t++) {
            if ((skip && skip[t]) || !lens[t] || blob[starts[t]] != (uint8_t)k) continue;
            ks[i] = starts[t];
            kl[i] = lens[t];
            kd[i] = (uint32_t)t;
            i++;
        }
        gf_status s = GF_OK;
        int kind = -1;                                    // of the batch decoders' shared plumbing; the LSOP codecs have none
        switch (codecs[k]) {
        case GF_CODEC_HUFFMAN: kind = KIND_HUFFMAN; break;
        case GF_CODEC_DEFLATE: kind = KIND_DEFLATE; break;
        case GF_CODEC_CANON_HUFFMAN: kind = KIND_CANON; break;
        case GF_CODEC_LSOP12:
        case GF_CODEC_LSOP08: {
            // (the LSOP host paths have stages of their own: the packings are gathered into one blob first, in parallel)
            std::vector<uint64_t> off(i + 1, 0);
            for (size_t j = 0; j < i; j++) off[j + 1] = off[j] + kl[j];
            std::vector<uint8_t> sub((size_t)off[i] + 16);
            parallelFor(i, [&](size_t j) { memcpy(sub.data() + off[j], blob + ks[j], kl[j]); });
            std::vector<int32_t> out(i * cells), sst(i);
            s = (codecs[k] == GF_CODEC_LSOP12 ? gf_lsop12_decode_batch_i32 : gf_lsop08_decode_batch_i32)(c, nRows, nCols, i, sub.data(), off.data(), out.data(), sst.data());
            if (s != GF_OK) return s;
            parallelFor(i, [&](size_t j) {
                st[kd[j]] = sst[j];
                if (sst[j] == GF_OK) memcpy(values + (size_t)kd[j] * cells, out.data() + j * cells, cells * 4);
            });
            break;
        }
        default: return GF_ERR_ARG;
        }
        if (kind >= 0) s = decodeBatchHostG(kind, c, nRows, nCols, i, blob, nullptr, ks.data(), kl.data(), kd.data(), values, st);
        if (s != GF_OK) return s;
    }
    return GF_OK;
}

extern "C" {

// ------------------------------------------------------------------ CodecDeflate (predictor + M32 on the GPU, Deflate on the host)

size_t gf_m32_default_stride(int nRows, int nCols)
{
    const size_t cells = (size_t)nRows * (size_t)nCols;
    return roundUp(cells + cells / 4 + 256, 16);
}

size_t gf_m32_max_stream(int nRows, int nCols) { return roundUp((size_t)6 * (size_t)nRows * (size_t)nCols + 32, 16); }

gf_status gf_deflate_encode_batch_i32(gf_context *c, int codecIndex, int nRows, int nCols, size_t nTiles, const int32_t *values,
                                      uint8_t *blob, size_t blobCap, uint64_t *offsets, uint8_t *predictors, int32_t *status)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1 || !values || !offsets || (!blob && blobCap)) return GF_ERR_ARG;
    std::vector<std::vector<uint8_t>> packs;
    std::vector<uint8_t> chosen;
    std::vector<int32_t> st;
    gf_status s = deflateEncodeBatchHost(c, codecIndex, nRows, nCols, nTiles, values, nullptr, packs, chosen, st);
    if (s != GF_OK) return s;
    uint64_t total = 0;
    for (size_t t = 0; t < nTiles; t++) {
        offsets[t] = total;
        if (st[t] == GF_OK) total += packs[t].size();
    }
    offsets[nTiles] = total;
    if (status) memcpy(status, st.data(), nTiles * 4);
    if (predictors) memcpy(predictors, chosen.data(), nTiles);
    if (total > blobCap) return GF_ERR_CAPACITY;
    for (size_t t = 0; t < nTiles; t++)
        if (st[t] == GF_OK) memcpy(blob + offsets[t], packs[t].data(), packs[t].size());
    return GF_OK;
}

// CodecDeflate.decode :108-155: the zlib stream of every packing is inflated ON THE DEVICE (gvrs_inflate.hip), the M32 bytes
// go through the decode kernel's raw mode; the host only moves bytes (chunked, pinned staging).
gf_status gf_deflate_decode_batch_i32(gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob,
                                      const uint64_t *offsets, int32_t *values, int32_t *status)
{
    GF_CTX_LOCK(c);
    return decodeBatchHost(KIND_DEFLATE, c, nRows, nCols, nTiles, blob, offsets, values, status);
}

gf_status gf_deflate_decode_batch_i32_dev(gf_context *c, void *stream, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob,
                                          size_t blobBytes, const uint64_t *dOffsets, size_t slotStride, const uint32_t *dLengths,
                                          int32_t *dValues, int32_t *dStatus)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1 || !dBlob || !dLengths || !dValues || !dStatus) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    return deflateDecodeDev(c, streamOf(c, stream), nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, slotStride,
                            dLengths, dValues, dStatus);
}

gf_status gf_deflate_encode_i32(gf_context *c, int codecIndex, int nRows, int nCols, const int32_t *values, uint8_t *out,
                                size_t outCap, size_t *outLen)
{
    GF_CTX_LOCK(c);
    return oneTileEncode(outLen, [&](uint64_t *offsets, int32_t *st) {
        return gf_deflate_encode_batch_i32(c, codecIndex, nRows, nCols, 1, values, out, outCap, offsets, nullptr, st);
    });
}

gf_status gf_deflate_decode_i32(gf_context *c, int nRows, int nCols, const uint8_t *packing, size_t len, int32_t *values)
{
    GF_CTX_LOCK(c);
    return oneTileDecode(len, [&](const uint64_t *offsets, int32_t *st) {
        return gf_deflate_decode_batch_i32(c, nRows, nCols, 1, packing, offsets, values, st);
    });
}


// ------------------------------------------------------------------ CodecMaster: the shortest packing over a codec list

// gvrs/CodecMaster.java:150-169 for a batch in host memory.  codecs[k] = GF_CODEC_* of the k-th entry of the file's codec list
// (GF_CODEC_NONE for an entry that has no integer encoder, e.g. CodecFloat); k is the codec index written to packing[0].
// Every integer codec encodes the batch; per tile the strictly shortest non-null packing wins, list order breaks ties.
gf_status gf_codec_master_encode_batch_i32(gf_context *c, const int *codecs, int nCodecs, int nRows, int nCols, size_t nTiles,
                                           const int32_t *values, uint8_t *blob, size_t blobCap, uint64_t *offsets,
                                           uint8_t *codecUsed, int32_t *status)
{
    GF_CTX_LOCK(c);
    if (!c || !codecs || nCodecs < 1 || nCodecs > 255 || !values || !offsets || (!blob && blobCap)) return GF_ERR_ARG;
    const size_t cells = (size_t)nRows * (size_t)nCols;
    for (int k = 0; k < nCodecs; k++)
        if (codecs[k] < GF_CODEC_NONE || codecs[k] > GF_CODEC_LSOP08) return GF_ERR_ARG;
    // per codec of the list: its packings (Deflate: one vector per tile; the others: one blob + offsets) and statuses
    struct Entry {
        std::unique_ptr<uint8_t[]> blob;
        std::vector<uint64_t> off;
        std::vector<std::vector<uint8_t>> packs;
        std::vector<int32_t> st;
        bool ran = false;
    };
    std::vector<Entry> e(nCodecs);
    auto lenOf = [&](int k, size_t t) -> size_t {
        const Entry &x = e[k];
        if (!x.ran || x.st[t] != GF_OK) return 0;
        return codecs[k] == GF_CODEC_DEFLATE ? x.packs[t].size() : (size_t)(x.off[t + 1] - x.off[t]);
    };
    // The GPU codecs first, CodecDeflate last: its three zlib streams per tile are the expensive part of the list, and a stream
    // that is already longer than what another codec of the list made of the tile cannot win (:161-164: the shortest packing
    // wins, the earlier codec on ties) -- deflateEncodeBatchHost gives such candidates up early.
    for (int pass = 0; pass < 2; pass++) {
        for (int k = 0; k < nCodecs; k++) {
            const int kind = codecs[k];
            if (kind == GF_CODEC_NONE || (kind == GF_CODEC_DEFLATE) != (pass == 1)) continue;
            Entry &x = e[k];
            x.st.assign(nTiles, GF_OK);
            gf_status s = GF_OK;
            if (kind == GF_CODEC_DEFLATE) {
                // what a Deflate packing may measure at most to be of use: strictly less than the codecs before it, no more than those behind
                std::vector<uint32_t> bound(nTiles, 0xFFFFFFFFu);
                for (size_t t = 0; t < nTiles; t++)
                    for (int j = 0; j < nCodecs; j++) {
                        const size_t len = j == k ? 0 : lenOf(j, t);
                        if (len) bound[t] = (uint32_t)std::min<size_t>(bound[t], j < k ? len - 1 : len);
                    }
                std::vector<uint8_t> chosen;
                s = deflateEncodeBatchHost(c, k, nRows, nCols, nTiles, values, bound.data(), x.packs, chosen, x.st);
            } else {
                x.off.assign(nTiles + 1, 0);
                size_t cap = nTiles * (cells + 1024) + 64;                       // a byte per cell holds terrain packings; grown once if not
                for (int attempt = 0; attempt < 2; attempt++) {
                    x.blob.reset(new uint8_t[cap]);
                    switch (kind) {
                    case GF_CODEC_HUFFMAN: s = gf_huffman_encode_batch_i32(c, k, nRows, nCols, nTiles, values, x.blob.get(), cap, x.off.data(), nullptr, x.st.data()); break;
                    case GF_CODEC_CANON_HUFFMAN: s = gf_canon_encode_batch_i32(c, k, nRows, nCols, nTiles, values, x.blob.get(), cap, x.off.data(), nullptr, x.st.data()); break;
                    case GF_CODEC_LSOP08: s = gf_lsop08_encode_batch_i32(c, k, nRows, nCols, nTiles, values, x.blob.get(), cap, x.off.data(), nullptr, x.st.data()); break;
                    default: s = gf_lsop12_encode_batch_i32(c, k, nRows, nCols, nTiles, values, 1, x.blob.get(), cap, x.off.data(), nullptr, x.st.data()); break;
                    }
                    if (s != GF_ERR_CAPACITY) break;
                    cap = (size_t)x.off[nTiles] + 64;
                }
            }
            if (s != GF_OK) return s;
            x.ran = true;
        }
    }
    // per tile the first shortest packing in list order; a tile no codec packed reports the first encoder error (the Java
    // encoder threw) or "declined"
    std::vector<int32_t> bestSt(nTiles, GF_DECLINED);
    std::vector<uint8_t> used(nTiles, 0xff);
    uint64_t total = 0;
    for (size_t t = 0; t < nTiles; t++) {
        size_t bestLen = 0;
        for (int k = 0; k < nCodecs; k++) {
            if (!e[k].ran) continue;
            const int32_t stK = e[k].st[t];
            if (stK < 0) { if (used[t] == 0xff && bestSt[t] >= 0) bestSt[t] = stK; continue; }
            const size_t len = lenOf(k, t);
            if (len && (used[t] == 0xff || len < bestLen)) {                     // strictly shorter (:161-164)
                bestLen = len;
                used[t] = (uint8_t)k;
                bestSt[t] = GF_OK;
            }
        }
        offsets[t] = total;
        total += bestLen;
    }
    offsets[nTiles] = total;
    if (status) memcpy(status, bestSt.data(), nTiles * 4);
    if (codecUsed) memcpy(codecUsed, used.data(), nTiles);
    if (total > blobCap) return GF_ERR_CAPACITY;
    parallelFor(nTiles, [&](size_t t) {
        if (bestSt[t] != GF_OK) return;
        const int k = used[t];
        const uint8_t *src = codecs[k] == GF_CODEC_DEFLATE ? e[k].packs[t].data() : e[k].blob.get() + e[k].off[t];
        memcpy(blob + offsets[t], src, (size_t)(offsets[t + 1] - offsets[t]));
    });
    return GF_OK;
}

gf_status gf_codec_master_decode_batch_i32(gf_context *c, const int *codecs, int nCodecs, int nRows, int nCols, size_t nTiles,
                                           const uint8_t *blob, const uint64_t *offsets, int32_t *values, int32_t *status)
{
    GF_CTX_LOCK(c);
    if (!c || !codecs || nCodecs < 1 || !blob || !offsets || !values) return GF_ERR_ARG;
    if (!offsetsValid(offsets, nTiles)) return GF_ERR_ARG;    // a bad array must not become an out-of-bounds read
    std::vector<int32_t> st(nTiles, GF_ERR_FORMAT);
    std::vector<uint32_t> lens(nTiles);
    for (size_t t = 0; t < nTiles; t++) lens[t] = (uint32_t)(offsets[t + 1] - offsets[t]);
    const gf_status s = codecMasterDecodeScattered(c, codecs, nCodecs, nRows, nCols, nTiles, blob, offsets, lens.data(), nullptr, values,
                                                   st.data());
    if (s != GF_OK) return s;
    if (status) memcpy(status, st.data(), nTiles * 4);
    return GF_OK;
}


// ------------------------------------------------------------------ tile payloads (one integer element per tile)

// RasterTile.getCompressedPacking (gvrs/RasterTile.java:234-256) over TileElementInt.encode (gvrs/TileElementInt.java:196-207)
// for a batch: per tile [int32 LE n][n bytes], the bytes being the CodecMaster packing, or the raw little-endian cells when
// no codec produced one or it is not shorter than them.  What RecordManager.writeTile stores behind the tile index.
gf_status gf_tile_payload_encode_batch_i32(gf_context *c, const int *codecs, int nCodecs, int nRows, int nCols, size_t nTiles,
                                           const int32_t *values, uint8_t *blob, size_t blobCap, uint64_t *offsets,
                                           uint8_t *codecUsed)
{
    GF_CTX_LOCK(c);
    if (!c || !values || !offsets || (!blob && blobCap)) return GF_ERR_ARG;
    const size_t cells = (size_t)nRows * (size_t)nCols, rawBytes = cells * 4;
    std::vector<uint8_t> packs(nTiles * (rawBytes + 1024) + 64);
    std::vector<uint64_t> off(nTiles + 1);
    std::vector<int32_t> st(nTiles);
    std::vector<uint8_t> used(nTiles);
    gf_status s = gf_codec_master_encode_batch_i32(c, codecs, nCodecs, nRows, nCols, nTiles, values, packs.data(), packs.size(),
                                                   off.data(), used.data(), st.data());
    if (s == GF_ERR_CAPACITY) {
        packs.resize((size_t)off[nTiles] + 64);
        s = gf_codec_master_encode_batch_i32(c, codecs, nCodecs, nRows, nCols, nTiles, values, packs.data(), packs.size(), off.data(),
                                             used.data(), st.data());
    }
    if (s != GF_OK) return s;
    uint64_t total = 0;
    for (size_t t = 0; t < nTiles; t++) {
        if (st[t] < 0) return (gf_status)st[t];                          // an encoder threw: the Java call fails as a whole
        const size_t n = st[t] == GF_OK ? (size_t)(off[t + 1] - off[t]) : 0;
        const bool raw = st[t] != GF_OK || n >= rawBytes;
        offsets[t] = total;
        total += 4 + (raw ? rawBytes : n);
        if (raw) used[t] = 0xff;
    }
    offsets[nTiles] = total;
    if (codecUsed) memcpy(codecUsed, used.data(), nTiles);
    if (total > blobCap) return GF_ERR_CAPACITY;
    for (size_t t = 0; t < nTiles; t++) {
        uint8_t *p = blob + offsets[t];
        const size_t n = (size_t)(offsets[t + 1] - offsets[t]) - 4;
        putLE32(p, (uint32_t)n);
        if (used[t] == 0xff) memcpy(p + 4, values + t * cells, rawBytes);   // little-endian host == the file's byte order
        else memcpy(p + 4, packs.data() + off[t], n);
    }
    return GF_OK;
}

// TileElementInt.decode (gvrs/TileElementInt.java:209-219): an encoding of exactly 4*cells bytes is the raw cells
gf_status gf_tile_payload_decode_batch_i32(gf_context *c, const int *codecs, int nCodecs, int nRows, int nCols, size_t nTiles,
                                           const uint8_t *blob, const uint64_t *offsets, int32_t *values, int32_t *status)
{
    GF_CTX_LOCK(c);
    if (!c || !blob || !offsets || !values) return GF_ERR_ARG;
    if (!offsetsValid(offsets, nTiles)) return GF_ERR_ARG;    // a bad array must not become an out-of-bounds read
    const size_t cells = (size_t)nRows * (size_t)nCols, rawBytes = cells * 4;
    std::vector<uint64_t> starts(nTiles, 0);
    std::vector<uint32_t> lens(nTiles, 0);
    std::vector<int32_t> st(nTiles, GF_OK);
    std::vector<uint8_t> skip(nTiles, 0);
    bool anyPacked = false;
    for (size_t t = 0; t < nTiles; t++) {
        const size_t len = (size_t)(offsets[t + 1] - offsets[t]);
        skip[t] = 1;
        if (len < 4) { st[t] = GF_ERR_BOUNDS; continue; }
        const size_t n = getLE32(blob + offsets[t]);
        if (n + 4 > len) { st[t] = GF_ERR_BOUNDS; continue; }
        starts[t] = offsets[t] + 4;
        lens[t] = (uint32_t)n;
        if (n == rawBytes) { skip[t] = 2; continue; }          // the cells themselves (copied below)
        skip[t] = 0;
        anyPacked = true;
    }
    parallelFor(nTiles, [&](size_t t) {
        if (skip[t] == 2) memcpy(values + t * cells, blob + starts[t], rawBytes);
    });
    if (anyPacked) {
        if (!codecs || nCodecs < 1) return GF_ERR_ARG;
        const gf_status s = codecMasterDecodeScattered(c, codecs, nCodecs, nRows, nCols, nTiles, blob, starts.data(), lens.data(), skip.data(),
                                                       values, st.data());
        if (s != GF_OK) return s;
    }
    if (status) memcpy(status, st.data(), nTiles * 4);
    return GF_OK;
}

}  // extern "C"
