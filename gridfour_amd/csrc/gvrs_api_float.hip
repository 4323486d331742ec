// gvrs_api_float.hip -- CodecFloat: the planes on the device, the host's zlib stage of the encoder, the inflating decoder; and
// gf_inflate_batch_dev.

#include "gvrs_api_internal.h"

// java.util.zip.Deflater(level): setInput, finish, deflate(.., FULL_FLUSH) == one complete zlib stream
bool zDeflate(const uint8_t *in, size_t n, int level, std::vector<uint8_t> &out)
{
    uLongf cap = compressBound((uLong)n) + 64;
    out.resize(cap);
    if (compress2(out.data(), &cap, in, (uLong)n, level) != Z_OK) return false;
    out.resize(cap);
    return true;
}

// The same stream, given up as soon as it is longer than `limit` bytes (returns false then, as on a zlib error): the caller only
// wants it if it is no longer than that.  Feeding the whole input with Z_FINISH and draining the output in pieces gives the bytes
// of compress2 -- what comes out of deflate() does not depend on how much room each call is given.
bool zDeflateUpTo(const uint8_t *in, size_t n, int level, size_t limit, std::vector<uint8_t> &out)
{
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (deflateInit(&zs, level) != Z_OK) return false;
    const size_t bound = (size_t)compressBound((uLong)n) + 64;
    out.resize(bound);
    zs.next_in = const_cast<Bytef *>(in);
    zs.avail_in = (uInt)n;
    size_t done = 0;
    int rc = Z_OK;
    while (rc == Z_OK) {
        const size_t room = std::min<size_t>(bound - done, 2048);
        zs.next_out = out.data() + done;
        zs.avail_out = (uInt)room;
        rc = deflate(&zs, Z_FINISH);
        done += room - zs.avail_out;
        if (done > limit && rc != Z_STREAM_END) { deflateEnd(&zs); return false; }
        if (room == 0) break;
    }
    deflateEnd(&zs);
    if (rc != Z_STREAM_END || done > limit) return false;
    out.resize(done);
    return true;
}

// CodecFloat packings decoded on the device: walk the packings, inflate their five streams (gvrs_inflate.hip), merge the planes -- in
// chunks of tiles through the bounded scratch, as deflateDecodeDev (gvrs_api_deflate.hip)
gf_status floatDecodeDev(gf_context *c, hipStream_t st, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob, size_t blobBytes,
                         const uint64_t *dOffsets, const uint32_t *dLengths, float *dValues, int32_t *dStatus)
{
    const size_t cells = (size_t)nRows * (size_t)nCols;
    if (cells >= (1ull << 28)) return GF_ERR_UNSUPPORTED;
    if (!dOffsets) return GF_ERR_ARG;
    const size_t planeStride = roundUp(gf_float_planes_bytes(nRows, nCols), 16);
    const size_t chunk = std::max<size_t>(1, std::min(nTiles, INFLATE_SCRATCH_BYTES / planeStride));
    gf_status s;
    if ((s = c->dInflOut.ensure(chunk * planeStride + 64)) != GF_OK) return s;
    if ((s = c->dInflate.ensure(chunk * 5 * sizeof(GfInflateStream) + 64)) != GF_OK) return s;
    if ((s = c->dInflMeta.ensure(chunk * (5 * 8 + 4) + 256)) != GF_OK) return s;
    uint8_t *planes = (uint8_t *)c->dInflOut.p;
    GfInflateStream *desc = (GfInflateStream *)c->dInflate.p;
    uint32_t *produced = (uint32_t *)c->dInflMeta.p;
    int32_t *inflStatus = (int32_t *)(produced + 5 * chunk), *pre = inflStatus + 5 * chunk;
    for (size_t t0 = 0; t0 < nTiles; t0 += chunk) {
        const size_t n = std::min(chunk, nTiles - t0);
        GF_HIP(hipMemsetAsync(planes, 0, n * planeStride, st));           // what a short stream does not reach reads as zero
        GF_HIP(gf_launch_float_streams(dBlob, blobBytes, dOffsets, dLengths, t0, n, (uint32_t)cells, planeStride, desc, pre, st));
        GfInflateArgs a{};
        a.inBase = dBlob;
        a.outBase = planes;
        a.streams = desc;
        a.produced = produced;
        a.status = inflStatus;
        a.nStreams = 5 * n;
        a.window = gf_inflate_window((uint32_t)std::min<size_t>(cells, 32768));
        GF_HIP(gf_launch_inflate(a, st));
        GF_HIP(gf_launch_float_short_planes(n, pre, inflStatus, produced, planes, planeStride, nRows, nCols, st));
        GF_HIP(gf_launch_float_status(n, pre, inflStatus, dStatus + t0, st));
        GF_HIP(gf_launch_float_planes_decode(planes, (uint32_t *)dValues + t0 * cells, planeStride, n, nRows, nCols, st));
    }
    return GF_OK;
}

extern "C" {

// ------------------------------------------------------------------ CodecFloat

size_t gf_float_planes_bytes(int nRows, int nCols)
{
    const size_t n = (size_t)nRows * (size_t)nCols;
    return (n + 7) / 8 + 4 * n;
}

gf_status gf_float_planes_encode_dev(gf_context *c, void *stream, int nRows, int nCols, size_t nTiles, const float *dValues,
                                     uint8_t *dPlanes, size_t planeStride)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1 || !dValues || !dPlanes || planeStride < gf_float_planes_bytes(nRows, nCols)) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    GF_HIP(gf_launch_float_planes_encode((const uint32_t *)dValues, dPlanes, planeStride, nTiles, nRows, nCols,
                                         streamOf(c, stream)));
    return GF_OK;
}

gf_status gf_float_planes_decode_dev(gf_context *c, void *stream, int nRows, int nCols, size_t nTiles, const uint8_t *dPlanes,
                                     size_t planeStride, float *dValues)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1 || !dValues || !dPlanes || planeStride < gf_float_planes_bytes(nRows, nCols)) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    GF_HIP(gf_launch_float_planes_decode(dPlanes, (uint32_t *)dValues, planeStride, nTiles, nRows, nCols,
                                         streamOf(c, stream)));
    return GF_OK;
}

gf_status gf_float_encode_batch_f32(gf_context *c, int codecIndex, int nRows, int nCols, size_t nTiles, const float *values,
                                    int zlibLevel, uint8_t *blob, size_t blobCap, uint64_t *offsets)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1 || !values || !offsets || (!blob && blobCap)) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)nRows * (size_t)nCols, nSign = (n + 7) / 8;
    const size_t stride = roundUp(gf_float_planes_bytes(nRows, nCols), 16);
    // staging: values | planes
    std::vector<uint8_t> planes(nTiles * stride);
    HostStage sg(c);
    const int valuesP = sg.in(values, nTiles * n * 4), planesP = sg.out(planes.data(), nTiles * stride);
    gf_status s = sg.begin();
    if (s != GF_OK) return s;
    s = gf_float_planes_encode_dev(c, c->stream, nRows, nCols, nTiles, sg.ptr<float>(valuesP), sg.ptr<uint8_t>(planesP), stride);
    if (s != GF_OK || (s = sg.end()) != GF_OK) return s;
    // framing, CodecFloat.java:371-391: codecIndex, 0, then five [int32 LE length, zlib stream]
    std::vector<std::vector<uint8_t>> packed(nTiles);
    std::vector<uint8_t> failed(nTiles, 0);
    parallelFor(nTiles, [&](size_t t) {
        const uint8_t *p = planes.data() + t * stride;
        std::vector<uint8_t> &out = packed[t];
        std::vector<uint8_t> z;
        out.push_back((uint8_t)codecIndex);
        out.push_back(0);
        size_t planeOff = 0;
        for (int k = 0; k < 5; k++) {
            const size_t pl = k == 0 ? nSign : n;
            if (!zDeflate(p + planeOff, pl, zlibLevel, z)) { failed[t] = 1; return; }
            planeOff += pl;
            const uint32_t zn = (uint32_t)z.size();
            for (int b = 0; b < 4; b++) out.push_back((uint8_t)(zn >> (8 * b)));
            out.insert(out.end(), z.begin(), z.end());
        }
    });
    uint64_t total = 0;
    for (size_t t = 0; t < nTiles; t++) {
        if (failed[t]) return GF_ERR_ARG;                     // zlib rejected the level
        offsets[t] = total;
        total += packed[t].size();
    }
    offsets[nTiles] = total;
    if (total > blobCap) return GF_ERR_CAPACITY;
    parallelFor(nTiles, [&](size_t t) { memcpy(blob + offsets[t], packed[t].data(), packed[t].size()); });
    return GF_OK;
}

// CodecFloat.decodeFloats :395-458 for a batch: the five zlib streams of every packing are inflated ON THE DEVICE
// (gvrs_inflate.hip), the planes merged there; the host only moves bytes (chunked, pinned staging).  Without a status array
// the first failing tile's status is the return value.
gf_status gf_float_decode_batch_f32(gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob,
                                    const uint64_t *offsets, float *values, int32_t *status)
{
    GF_CTX_LOCK(c);
    if (status) return decodeBatchHost(KIND_FLOAT, c, nRows, nCols, nTiles, blob, offsets, (int32_t *)values, status);
    std::vector<int32_t> st(nTiles, GF_OK);
    const gf_status s = decodeBatchHost(KIND_FLOAT, c, nRows, nCols, nTiles, blob, offsets, (int32_t *)values, st.data());
    if (s != GF_OK) return s;
    for (size_t t = 0; t < nTiles; t++)
        if (st[t] != GF_OK) return (gf_status)st[t];
    return GF_OK;
}

gf_status gf_float_decode_batch_f32_dev(gf_context *c, void *stream, int nRows, int nCols, size_t nTiles, const uint8_t *dBlob,
                                        size_t blobBytes, const uint64_t *dOffsets, const uint32_t *dLengths, float *dValues,
                                        int32_t *dStatus)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1 || !dBlob || !dOffsets || !dLengths || !dValues || !dStatus) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    return floatDecodeDev(c, streamOf(c, stream), nRows, nCols, nTiles, dBlob, blobBytes, dOffsets, dLengths, dValues, dStatus);
}

gf_status gf_float_encode_f32(gf_context *c, int codecIndex, int nRows, int nCols, const float *values, int zlibLevel,
                              uint8_t *out, size_t outCap, size_t *outLen)
{
    GF_CTX_LOCK(c);
    return oneTileEncode(outLen, [&](uint64_t *offsets, int32_t *) {           // (CodecFloat has no tile status of its own)
        return gf_float_encode_batch_f32(c, codecIndex, nRows, nCols, 1, values, zlibLevel, out, outCap, offsets);
    });
}

gf_status gf_float_decode_f32(gf_context *c, int nRows, int nCols, const uint8_t *packing, size_t len, float *values)
{
    GF_CTX_LOCK(c);
    return oneTileDecode(len, [&](const uint64_t *offsets, int32_t *st) {
        return gf_float_decode_batch_f32(c, nRows, nCols, 1, packing, offsets, values, st);
    });
}

// zlib streams inflated on the device (gvrs_inflate.hip): stream i = d_in[in_offsets[i] .. + in_lengths[i]) -> at most out_caps[i]
// bytes at d_out + out_offsets[i].  The four descriptor arrays are HOST arrays (they are packed and uploaded here);
// d_produced / d_status are device arrays.  Enqueues only (after the small descriptor upload on the same stream).
gf_status gf_inflate_batch_dev(gf_context *c, void *stream, size_t nStreams, const uint8_t *dIn, const uint64_t *inOffsets,
                               const uint32_t *inLengths, uint8_t *dOut, const uint64_t *outOffsets, const uint32_t *outCaps,
                               uint32_t *dProduced, int32_t *dStatus)
{
    GF_CTX_LOCK(c);
    if (!c || (nStreams && (!dIn || !inOffsets || !inLengths || !dOut || !outOffsets || !outCaps || !dProduced || !dStatus)))
        return GF_ERR_ARG;
    if (nStreams == 0) return GF_OK;
    GF_HIP(hipSetDevice(c->device));
    const hipStream_t st = streamOf(c, stream);
    gf_status s = c->dInflate.ensure(nStreams * sizeof(GfInflateStream) + 16);
    if (s != GF_OK) return s;
    std::vector<GfInflateStream> desc(nStreams);
    uint32_t maxCap = 0;
    for (size_t i = 0; i < nStreams; i++) {
        desc[i].inOffset = inOffsets[i];
        desc[i].outOffset = outOffsets[i];
        desc[i].inLen = inLengths[i];
        desc[i].outCap = outCaps[i];
        maxCap = std::max(maxCap, outCaps[i]);
    }
    // (pageable source: the copy is staged by the runtime before the call returns)
    GF_HIP(hipMemcpyAsync(c->dInflate.p, desc.data(), nStreams * sizeof(GfInflateStream), hipMemcpyHostToDevice, st));
    GfInflateArgs a{};
    a.inBase = dIn;
    a.outBase = dOut;
    a.streams = (const GfInflateStream *)c->dInflate.p;
    a.produced = dProduced;
    a.status = dStatus;
    a.nStreams = nStreams;
    a.window = gf_inflate_window(maxCap);
    GF_HIP(gf_launch_inflate(a, st));
    return GF_OK;
}

}  // extern "C"
