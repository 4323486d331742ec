// gvrs_api_host.hip -- the host-memory entry points of CodecHuffman and CodecCanonHuffman: the pipelined staging of a batch and
// the one-tile-per-call path with its recorded graphs.

#include "gvrs_api_internal.h"

// ---- pipelined staging of the host-memory batch entry points ---------------------------------------------------
// A batch in host memory is cut into chunks of about HOST_CHUNK_BYTES of cell values.  Each chunk travels through one of
// HOST_SLOTS slots (pinned staging buffers, device buffers, a stream of its own): the calling thread copies the caller's
// (pageable) memory into the slot's pinned buffer with a few helper threads, enqueues H2D copy + kernels + D2H copy on the
// slot's stream and moves on to the next chunk, so that the copy-in of chunk k+1, the device work of chunk k and the
// copy-out of chunk k-1 overlap.  Device and pinned memory are bounded by the chunk, not by the batch.  Memory the caller
// obtained from gf_host_alloc (or pinned itself) is used in place, without the staging copy.
constexpr int HOST_SLOTS = 3;
constexpr size_t HOST_CHUNK_BYTES = (size_t)64 << 20;

struct HostSlot {
    hipStream_t stream = nullptr;
    hipEvent_t evA = nullptr, evB = nullptr;       // device work enqueued so far / final copy-out done
    hipEvent_t evK = nullptr;                      // the chunk's codec kernels are done (they use the context's per-tile records)
    DevBuf dValues, dSlots, dBlob, dLengths, dPred, dStatus, dOffsets;
    PinBuf hIn, hOut, hMeta;
    void release()
    {
        dValues.release(); dSlots.release(); dBlob.release(); dLengths.release(); dPred.release(); dStatus.release();
        dOffsets.release(); hIn.release(); hOut.release(); hMeta.release();
        if (evA) (void)hipEventDestroy(evA);
        if (evB) (void)hipEventDestroy(evB);
        if (evK) (void)hipEventDestroy(evK);
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr; evA = evB = evK = nullptr;
    }
};

struct gf_host_pipe {
    HostSlot slot[HOST_SLOTS];
};

static gf_status hostPipe(gf_context *c, gf_host_pipe **out)
{
    if (!c->pipe) {
        gf_host_pipe *p = new (std::nothrow) gf_host_pipe();
        if (!p) return GF_ERR_ARG;
        for (int i = 0; i < HOST_SLOTS; i++) {
            hipError_t e = hipStreamCreateWithFlags(&p->slot[i].stream, hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&p->slot[i].evA, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&p->slot[i].evB, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&p->slot[i].evK, hipEventDisableTiming);
            if (e != hipSuccess) {
                for (int j = 0; j <= i; j++) p->slot[j].release();
                delete p;
                return hipFail(e, "host pipeline set-up");
            }
        }
        c->pipe = p;
    }
    *out = c->pipe;
    return GF_OK;
}

void gf_host_pipe_destroy(gf_host_pipe *p)
{
    if (!p) return;
    for (int i = 0; i < HOST_SLOTS; i++) p->slot[i].release();
    delete p;
}

// is this host pointer page-locked (hipHostMalloc / hipHostRegister)?  Then the DMA engines read and write it directly.
static bool isPinned(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();                   // pageable memory is reported as an error; clear it
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

// memcpy with a few helper threads: one thread moves 6-10 GB/s, PCIe Gen5 x16 five times that
static void parallelCopy(void *dst, const void *src, size_t bytes)
{
    const size_t per = (size_t)8 << 20;
    unsigned nt = (unsigned)std::min<size_t>(8, bytes / per);
    const unsigned hw = std::thread::hardware_concurrency();
    if (hw && nt > hw) nt = hw;
    if (nt <= 1) { memcpy(dst, src, bytes); return; }
    const size_t part = roundUp((bytes + nt - 1) / nt, 4096);
    std::vector<std::thread> th;
    for (unsigned w = 1; w < nt; w++) {
        const size_t o = (size_t)w * part;
        if (o >= bytes) break;
        th.emplace_back([=]() { memcpy((uint8_t *)dst + o, (const uint8_t *)src + o, std::min(part, bytes - o)); });
    }
    memcpy(dst, src, std::min(part, bytes));
    for (auto &x : th) x.join();
}

// The pinned meta record of a chunk (HostSlot::hMeta): offsets[chunk + 1], lengths[chunk], statuses[chunk] and -- the encoder's only --
// predictors[chunk], each from a 64-byte boundary.
struct HostMeta {
    Carve k;
    const size_t offAt, lenAt, stAt, predAt;
    uint64_t *off = nullptr;
    uint32_t *len = nullptr;
    int32_t *st = nullptr;
    uint8_t *pred = nullptr;
    HostMeta(size_t chunk, bool predictors)
        : offAt(k.add((chunk + 1) * 8, 64)), lenAt(k.add(chunk * 4, 64)), stAt(k.add(chunk * 4, 64)), predAt(k.add(predictors ? chunk : 0, 64))
    {
    }
    // the parts in a slot's record (which holds at least this layout: the encoder's has the predictors behind the decoder's)
    HostMeta(const HostSlot &S, size_t chunk) : HostMeta(chunk, true)
    {
        off = S.hMeta.at<uint64_t>(offAt), len = S.hMeta.at<uint32_t>(lenAt), st = S.hMeta.at<int32_t>(stAt), pred = S.hMeta.at<uint8_t>(predAt);
    }
};

static size_t hostChunkTiles(size_t cells, size_t nTiles, int kind = KIND_HUFFMAN)
{
    // the inflate kernels run one wave per zlib stream and a stream is a serial chain: a chunk has to bring thousands of streams
    const size_t bytes = kind == KIND_DEFLATE || kind == KIND_FLOAT ? 4 * HOST_CHUNK_BYTES : HOST_CHUNK_BYTES;
    const size_t n = std::max<size_t>(1, bytes / (cells * 4));
    return std::min(n, std::max<size_t>(nTiles, 1));
}

static gf_status encodeBatchHost(int kind, gf_context *c, int codecIndex, int nRows, int nCols, size_t nTiles,
                                 const int32_t *values, uint8_t *blob, size_t blobCap, uint64_t *offsets,
                                 uint8_t *predictors, int32_t *status)
{
    if (!c || nRows < 1 || nCols < 1 || (!values && nTiles) || !offsets || (!blob && blobCap)) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    gf_host_pipe *P;
    gf_status s = hostPipe(c, &P);
    if (s != GF_OK) return s;
    const size_t cells = (size_t)nRows * (size_t)nCols;
    const size_t stride = gf_huffman_default_stride(nRows, nCols);
    const size_t chunk = hostChunkTiles(cells, nTiles);
    const size_t nChunks = (nTiles + chunk - 1) / chunk;
    const bool pinnedIn = nTiles && isPinned(values);
    // the per-tile records between the encoder kernels are per context: one launch at a time uses them, so every chunk's
    // kernels run in the context's stream order (the slot streams carry the copies and wait for / signal the kernels)
    if ((s = gf_context_reserve(c, nRows, nCols, chunk)) != GF_OK) return s;

    for (int i = 0; i < HOST_SLOTS && (size_t)i < nChunks; i++) {
        HostSlot &S = P->slot[i];
        if ((s = S.dValues.ensure(chunk * cells * 4 + 16)) != GF_OK) return s;
        if ((s = S.dSlots.ensure(chunk * stride + 16)) != GF_OK) return s;
        if ((s = S.dBlob.ensure(chunk * stride + 16)) != GF_OK) return s;
        if ((s = S.dLengths.ensure(chunk * 4 + 16)) != GF_OK) return s;
        if ((s = S.dPred.ensure(chunk + 16)) != GF_OK) return s;
        if ((s = S.dStatus.ensure(chunk * 4 + 16)) != GF_OK) return s;
        if ((s = S.dOffsets.ensure((chunk + 1) * 8 + 16)) != GF_OK) return s;
        if (!pinnedIn && (s = S.hIn.ensure(chunk * cells * 4)) != GF_OK) return s;
        if ((s = S.hOut.ensure(chunk * stride)) != GF_OK) return s;
        if ((s = S.hMeta.ensure(HostMeta(chunk, true).k, 64)) != GF_OK) return s;
    }

    uint64_t total = 0;                            // bytes of the packings placed so far
    bool overCap = false;
    offsets[0] = 0;
    // stage B of a chunk: its kernels are done -> overflow tiles, then the compact blob comes home
    auto stageB = [&](size_t k) -> gf_status {
        HostSlot &S = P->slot[k % HOST_SLOTS];
        const size_t t0 = k * chunk, n = std::min(chunk, nTiles - t0);
        const HostMeta m(S, chunk);
        GF_HIP(hipEventSynchronize(S.evA));
        const uint64_t bytes = m.off[n];
        if (bytes) GF_HIP(hipMemcpyAsync(S.hOut.p, S.dBlob.p, bytes, hipMemcpyDeviceToHost, S.stream));
        GF_HIP(hipEventRecord(S.evB, S.stream));
        return GF_OK;
    };
    // stage C: the blob of the chunk is in pinned memory -> the caller's arrays
    auto stageC = [&](size_t k) -> gf_status {
        HostSlot &S = P->slot[k % HOST_SLOTS];
        const size_t t0 = k * chunk, n = std::min(chunk, nTiles - t0);
        const HostMeta m(S, chunk);
        GF_HIP(hipEventSynchronize(S.evB));
        bool anyBig = false;
        for (size_t t = 0; t < n; t++) anyBig = anyBig || m.st[t] == GF_OVERFLOW;
        if (!anyBig) {
            const uint64_t bytes = m.off[n];
            if (total + bytes <= blobCap) {
                if (bytes) parallelCopy(blob + total, S.hOut.p, bytes);
            } else {
                overCap = true;
            }
            for (size_t t = 0; t < n; t++) offsets[t0 + t + 1] = total + m.off[t + 1];
            total += bytes;
        } else {
            // tiles whose packing did not fit the default slot (longer than the raw tile): redone one by one into a
            // worst-case slot so that the bytes are still exactly the reference's
            const size_t maxp = kind == KIND_CANON ? gf_canon_max_packing(nRows, nCols) : gf_huffman_max_packing(nRows, nCols);
            DevBuf slot, meta;
            gf_status r;
            for (int i = 0; i < HOST_SLOTS; i++) GF_HIP(hipStreamSynchronize(P->slot[i].stream));   // nothing else uses the records now
            if ((r = slot.ensure(maxp)) != GF_OK) return r;
            if ((r = meta.ensure(64)) != GF_OK) { slot.release(); return r; }
            std::vector<uint8_t> big;
            for (size_t t = 0; t < n; t++) {
                uint64_t len = (m.st[t] == GF_OK) ? m.len[t] : 0;
                const uint8_t *src = (const uint8_t *)S.hOut.p + m.off[t];
                if (m.st[t] == GF_OVERFLOW) {
                    uint32_t *dLen = (uint32_t *)meta.p;
                    int32_t *dSt = (int32_t *)((uint8_t *)meta.p + 16);
                    r = encodeBatchDev(kind, c, S.stream, codecIndex, nRows, nCols, 1, (const int32_t *)S.dValues.p + t * cells,
                                       (uint8_t *)slot.p, maxp, dLen, nullptr, dSt, GF_PM_ALL, 0);
                    uint32_t l = 0;
                    int32_t tst = 0;
                    hipError_t e = hipSuccess;
                    if (r == GF_OK) e = hipMemcpyAsync(&l, dLen, 4, hipMemcpyDeviceToHost, S.stream);
                    if (r == GF_OK && e == hipSuccess) e = hipMemcpyAsync(&tst, dSt, 4, hipMemcpyDeviceToHost, S.stream);
                    if (r == GF_OK && e == hipSuccess) e = hipStreamSynchronize(S.stream);
                    if (r == GF_OK && e == hipSuccess) {
                        big.resize(l);
                        if (l) e = hipMemcpy(big.data(), slot.p, l, hipMemcpyDeviceToHost);
                    }
                    if (r != GF_OK || e != hipSuccess) {
                        slot.release();
                        meta.release();
                        return r != GF_OK ? r : hipFail(e, "overflow tile copy");
                    }
                    m.st[t] = tst;
                    m.len[t] = l;
                    len = tst == GF_OK ? l : 0;
                    src = big.data();
                }
                if (total + len <= blobCap) {
                    if (len) memcpy(blob + total, src, len);
                } else {
                    overCap = true;
                }
                total += len;
                offsets[t0 + t + 1] = total;
            }
            slot.release();
            meta.release();
        }
        if (status) memcpy(status + t0, m.st, n * 4);
        if (predictors) memcpy(predictors + t0, m.pred, n);
        return GF_OK;
    };

    for (size_t k = 0; k < nChunks + 2; k++) {
        if (k >= 2 && k - 2 < nChunks && (s = stageC(k - 2)) != GF_OK) return s;     // frees slot (k - 2) % 3 ... used again at k + 1
        if (k < nChunks) {
            HostSlot &S = P->slot[k % HOST_SLOTS];
            const size_t t0 = k * chunk, n = std::min(chunk, nTiles - t0);
            const HostMeta m(S, chunk);
            const int32_t *src = values + t0 * cells;
            if (!pinnedIn) {
                parallelCopy(S.hIn.p, src, n * cells * 4);
                src = (const int32_t *)S.hIn.p;
            }
            GF_HIP(hipMemcpyAsync(S.dValues.p, src, n * cells * 4, hipMemcpyHostToDevice, S.stream));
            // the codec kernels of successive chunks share the context's per-tile records: they run one after the other
            // (the copies around them overlap freely)
            if (k > 0) GF_HIP(hipStreamWaitEvent(S.stream, P->slot[(k - 1) % HOST_SLOTS].evK, 0));
            s = encodeBatchDev(kind, c, S.stream, codecIndex, nRows, nCols, n, (const int32_t *)S.dValues.p, (uint8_t *)S.dSlots.p,
                               stride, (uint32_t *)S.dLengths.p, (uint8_t *)S.dPred.p, (int32_t *)S.dStatus.p, GF_PM_ALL, 0);
            if (s != GF_OK) return s;
            GF_HIP(hipEventRecord(S.evK, S.stream));
            GF_HIP(hipMemcpyAsync(m.len, S.dLengths.p, n * 4, hipMemcpyDeviceToHost, S.stream));
            GF_HIP(hipMemcpyAsync(m.st, S.dStatus.p, n * 4, hipMemcpyDeviceToHost, S.stream));
            GF_HIP(hipMemcpyAsync(m.pred, S.dPred.p, n, hipMemcpyDeviceToHost, S.stream));
            GF_HIP(gf_launch_compact(n, (const uint8_t *)S.dSlots.p, stride, (const uint32_t *)S.dLengths.p, (uint64_t *)S.dOffsets.p,
                                     (uint8_t *)S.dBlob.p, S.dBlob.bytes, S.stream, (const int32_t *)S.dStatus.p));
            GF_HIP(hipMemcpyAsync(m.off, S.dOffsets.p, (n + 1) * 8, hipMemcpyDeviceToHost, S.stream));
            GF_HIP(hipEventRecord(S.evA, S.stream));
        }
        if (k >= 1 && k - 1 < nChunks && (s = stageB(k - 1)) != GF_OK) return s;
    }
    return overCap ? GF_ERR_CAPACITY : GF_OK;
}

// The pipelined host-memory decode.  Packing t is lens[t] bytes at blob + starts[t] (starts / lens null: the usual offsets array,
// packings back to back) and its cells go to tile dstTile[t] of `values`, its status to status[dstTile[t]] (dstTile null: t).
// The scattered form (round 4) is what the default-codec-list and tile-record readers use: the packings of one codec among a
// batch's, or the elements inside framed records, are gathered straight into the pinned staging buffer of their chunk and the
// decoded tiles leave the staging buffer for their own place -- no intermediate blob, no intermediate tile array.
gf_status decodeBatchHostG(int kind, gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob, const uint64_t *offsets,
                           const uint64_t *starts, const uint32_t *lens, const uint32_t *dstTile, int32_t *values, int32_t *status)
{
    if (!c || nRows < 1 || nCols < 1 || !blob || (!offsets && !(starts && lens)) || (!values && nTiles)) return GF_ERR_ARG;
    if (!starts && !offsetsValid(offsets, nTiles)) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    gf_host_pipe *P;
    gf_status s = hostPipe(c, &P);
    if (s != GF_OK) return s;
    const size_t cells = (size_t)nRows * (size_t)nCols;
    const size_t chunk = hostChunkTiles(cells, nTiles, kind);
    const size_t nChunks = (nTiles + chunk - 1) / chunk;
    const bool pinnedOut = nTiles && !dstTile && isPinned(values);
    if ((s = gf_context_reserve(c, nRows, nCols, chunk)) != GF_OK) return s;
    auto lenOf = [&](size_t t) -> uint64_t { return starts ? (uint64_t)lens[t] : offsets[t + 1] - offsets[t]; };
    // the largest blob slice of a chunk
    uint64_t maxSlice = 0;
    for (size_t k = 0; k < nChunks; k++) {
        const size_t t0 = k * chunk, t1 = std::min(nTiles, t0 + chunk);
        uint64_t slice = 0;
        if (starts)
            for (size_t t = t0; t < t1; t++) slice += lens[t];
        else slice = offsets[t1] - offsets[t0];
        maxSlice = std::max(maxSlice, slice);
    }
    for (int i = 0; i < HOST_SLOTS && (size_t)i < nChunks; i++) {
        HostSlot &S = P->slot[i];
        if ((s = S.dValues.ensure(chunk * cells * 4 + 16)) != GF_OK) return s;
        if ((s = S.dBlob.ensure(maxSlice + 64)) != GF_OK) return s;
        if ((s = S.dLengths.ensure(chunk * 4 + 16)) != GF_OK) return s;
        if ((s = S.dStatus.ensure(chunk * 4 + 16)) != GF_OK) return s;
        if ((s = S.dOffsets.ensure((chunk + 1) * 8 + 16)) != GF_OK) return s;
        if ((s = S.hIn.ensure(maxSlice + 64)) != GF_OK) return s;
        if (!pinnedOut && (s = S.hOut.ensure(chunk * cells * 4)) != GF_OK) return s;
        if ((s = S.hMeta.ensure(HostMeta(chunk, false).k, 64)) != GF_OK) return s;
    }
    auto finish = [&](size_t k) -> gf_status {
        HostSlot &S = P->slot[k % HOST_SLOTS];
        const size_t t0 = k * chunk, n = std::min(chunk, nTiles - t0);
        GF_HIP(hipEventSynchronize(S.evA));
        const int32_t *st = HostMeta(S, chunk).st;
        if (dstTile) {
            const int32_t *src = (const int32_t *)S.hOut.p;
            parallelFor(n, [&](size_t t) {
                if (st[t] == GF_OK) memcpy(values + (size_t)dstTile[t0 + t] * cells, src + t * cells, cells * 4);
                if (status) status[dstTile[t0 + t]] = st[t];
            });
            return GF_OK;
        }
        if (!pinnedOut) parallelCopy(values + t0 * cells, S.hOut.p, n * cells * 4);
        if (status) memcpy(status + t0, st, n * 4);
        return GF_OK;
    };
    for (size_t k = 0; k < nChunks + (HOST_SLOTS - 1); k++) {
        if (k >= (size_t)(HOST_SLOTS - 1) && (s = finish(k - (HOST_SLOTS - 1))) != GF_OK) return s;
        if (k >= nChunks) continue;
        HostSlot &S = P->slot[k % HOST_SLOTS];
        const size_t t0 = k * chunk, n = std::min(chunk, nTiles - t0);
        const HostMeta m(S, chunk);                                          // (m.off: offsets inside the chunk's slice)
        uint64_t bytes = 0;
        for (size_t t = 0; t < n; t++) {
            m.off[t] = bytes;
            m.len[t] = (uint32_t)lenOf(t0 + t);
            bytes += m.len[t];
        }
        m.off[n] = bytes;
        if (bytes && !starts) memcpy(S.hIn.p, blob + offsets[t0], bytes);    // the slice starts 4-byte aligned in the staging buffer
        if (bytes && starts) {
            uint8_t *dst = (uint8_t *)S.hIn.p;
            parallelFor(n, [&](size_t t) { memcpy(dst + m.off[t], blob + starts[t0 + t], m.len[t]); });
        }
        if (bytes) GF_HIP(hipMemcpyAsync(S.dBlob.p, S.hIn.p, bytes, hipMemcpyHostToDevice, S.stream));
        GF_HIP(hipMemcpyAsync(S.dOffsets.p, m.off, (n + 1) * 8, hipMemcpyHostToDevice, S.stream));
        GF_HIP(hipMemcpyAsync(S.dLengths.p, m.len, n * 4, hipMemcpyHostToDevice, S.stream));
        if (k > 0) GF_HIP(hipStreamWaitEvent(S.stream, P->slot[(k - 1) % HOST_SLOTS].evK, 0));   // kernels one chunk at a time
        if (kind == KIND_DEFLATE)
            s = deflateDecodeDev(c, S.stream, nRows, nCols, n, (const uint8_t *)S.dBlob.p, bytes + 32, (const uint64_t *)S.dOffsets.p, 0,
                                 (const uint32_t *)S.dLengths.p, (int32_t *)S.dValues.p, (int32_t *)S.dStatus.p);
        else if (kind == KIND_FLOAT)
            s = floatDecodeDev(c, S.stream, nRows, nCols, n, (const uint8_t *)S.dBlob.p, bytes + 32, (const uint64_t *)S.dOffsets.p,
                               (const uint32_t *)S.dLengths.p, (float *)S.dValues.p, (int32_t *)S.dStatus.p);
        else
            s = decodeBatchDev(kind, c, S.stream, nRows, nCols, n, (const uint8_t *)S.dBlob.p, bytes + 32, (const uint64_t *)S.dOffsets.p, 0,
                               (const uint32_t *)S.dLengths.p, (int32_t *)S.dValues.p, (int32_t *)S.dStatus.p, 0);
        if (s != GF_OK) return s;
        GF_HIP(hipEventRecord(S.evK, S.stream));
        GF_HIP(hipMemcpyAsync(pinnedOut ? (void *)(values + t0 * cells) : S.hOut.p, S.dValues.p, n * cells * 4, hipMemcpyDeviceToHost,
                              S.stream));
        GF_HIP(hipMemcpyAsync(m.st, S.dStatus.p, n * 4, hipMemcpyDeviceToHost, S.stream));
        GF_HIP(hipEventRecord(S.evA, S.stream));
    }
    return GF_OK;
}

gf_status decodeBatchHost(int kind, gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob, const uint64_t *offsets,
                          int32_t *values, int32_t *status)
{
    if (!offsets) return GF_ERR_ARG;
    return decodeBatchHostG(kind, c, nRows, nCols, nTiles, blob, offsets, nullptr, nullptr, nullptr, values, status);
}

// ------------------------------------------------------------------ one tile per call (BASELINE config 1)
// What a stock Gridfour application reaches without a patched GvrsFile: CodecMaster hands a codec ONE tile per call
// (gvrs/CodecMaster.java:150-169, RasterTileCache.java:418-421).  Through the batch machinery that was 180-190 us per tile on an
// MI355X (three stream slots, five asynchronous copies, events, a dozen API calls) against 10-20 us of kernels.  Here (round 4):
// per context a page-locked input and output buffer and, per (direction, codec, tile shape, codec index), ONE hipGraph recorded
// from the same device entry points the batches use -- host-to-device copy of the input, the kernels; the outputs (packing,
// length, status / cells, status) are written by the kernels straight into the page-locked output buffer -- replayed with one
// launch and waited for by polling the stream.  The first call of a kind takes the batch path; the second runs the lean sequence
// once outside a capture (code objects of the 1,024-thread builds, the kernels' LDS attributes: what a capture must not do) and
// records the graph.  A capture that fails is remembered (the batch path from then on); graphs are recorded again when a device
// buffer they hold has moved (gf_context::bufMoves).
struct gf_single_graph {
    int dir, kind, nRows, nCols, codecIndex;
    size_t copyBytes;
    hipGraph_t graph;
    hipGraphExec_t exec;
};
struct gf_single {
    void *hIn = nullptr, *hOut = nullptr;
    size_t hInBytes = 0, hOutBytes = 0;
    DevBuf dIn;
    std::vector<gf_single_graph> graphs;
    uint64_t moves = 0;                                          // gf_context::bufMoves when the graphs were recorded
    std::vector<std::pair<int, std::pair<int, int>>> warmed;     // (dir * 8 + kind, shape) that ran once through the batch path
    std::vector<std::pair<int, std::pair<int, int>>> refused;    // ... whose capture failed: the batch path from then on
};
static void singleDropGraphs(gf_single *sg)
{
    for (auto &g : sg->graphs) {
        (void)hipGraphExecDestroy(g.exec);
        (void)hipGraphDestroy(g.graph);
    }
    sg->graphs.clear();
}
// The graphs hold device addresses of the context's buffers (tree / selection records, flags, workspace, dIn): when any device
// buffer of the context has moved since they were recorded, they are recorded again.
static gf_status singleCheckMoves(gf_context *c, gf_single *sg)
{
    const uint64_t now = c->bufMoves.load(std::memory_order_relaxed);
    if (sg->moves == now || sg->graphs.empty()) {
        sg->moves = now;
        return GF_OK;
    }
    GF_HIP(hipStreamSynchronize(c->stream));
    singleDropGraphs(sg);
    sg->moves = now;
    return GF_OK;
}
static bool singleRefused(gf_single *sg, int key, int nRows, int nCols, bool add = false)
{
    for (auto &w : sg->refused)
        if (w.first == key && w.second.first == nRows && w.second.second == nCols) return true;
    if (add) sg->refused.push_back({key, {nRows, nCols}});
    return false;
}
void gf_single_destroy(gf_single *sg)
{
    if (!sg) return;
    singleDropGraphs(sg);
    if (sg->hIn) (void)hipHostFree(sg->hIn);
    if (sg->hOut) (void)hipHostFree(sg->hOut);
    sg->dIn.release();
    delete sg;
}
static gf_status singleEnsure(gf_context *c, size_t inBytes, size_t outBytes)
{
    if (!c->single) {
        c->single = new (std::nothrow) gf_single;
        if (c->single) c->single->dIn.moves = &c->bufMoves;
    }
    gf_single *sg = c->single;
    if (!sg) return GF_ERR_HIP;
    if (sg->hInBytes < inBytes || sg->hOutBytes < outBytes || sg->dIn.bytes < inBytes) {
        // the graphs hold the old addresses
        GF_HIP(hipStreamSynchronize(c->stream));
        singleDropGraphs(sg);
        if (sg->hInBytes < inBytes) {
            if (sg->hIn) (void)hipHostFree(sg->hIn);
            sg->hIn = nullptr;
            sg->hInBytes = 0;
            GF_HIP(hipHostMalloc(&sg->hIn, roundUp(inBytes, 4096), hipHostMallocDefault));
            sg->hInBytes = roundUp(inBytes, 4096);
        }
        if (sg->hOutBytes < outBytes) {
            if (sg->hOut) (void)hipHostFree(sg->hOut);
            sg->hOut = nullptr;
            sg->hOutBytes = 0;
            GF_HIP(hipHostMalloc(&sg->hOut, roundUp(outBytes, 4096), hipHostMallocDefault));
            sg->hOutBytes = roundUp(outBytes, 4096);
        }
        const gf_status s = sg->dIn.ensure(inBytes);
        if (s != GF_OK) return s;
    }
    return GF_OK;
}
static bool singleWarmed(gf_single *sg, int key, int nRows, int nCols)
{
    for (auto &w : sg->warmed)
        if (w.first == key && w.second.first == nRows && w.second.second == nCols) return true;
    sg->warmed.push_back({key, {nRows, nCols}});
    return false;
}
// waits for the stream without the interrupt path of hipStreamSynchronize (tens of microseconds on its own)
static gf_status singleWait(hipStream_t st)
{
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e == hipSuccess) return GF_OK;
        if (e != hipErrorNotReady) {
            g_lastError = hipGetErrorString(e);
            return GF_ERR_HIP;
        }
    }
}

// The recorded graph of `want` (direction, codec, tile shape, codec index, copy size); where there is none yet it is recorded from
// `sequence`, the lean path's enqueue calls on c->stream.  GF_ERR_UNSUPPORTED where the capture failed.
template <class Sequence>
static gf_status singleGraph(gf_context *c, gf_single_graph want, Sequence sequence, gf_single_graph **out)
{
    gf_single *sg = c->single;
    for (auto &x : sg->graphs)
        if (x.dir == want.dir && x.kind == want.kind && x.nRows == want.nRows && x.nCols == want.nCols &&
            x.codecIndex == want.codecIndex && x.copyBytes == want.copyBytes) {
            *out = &x;
            return GF_OK;
        }
    gf_status s;
    if ((s = gf_context_reserve(c, want.nRows, want.nCols, 1)) != GF_OK) return s;
    const uint64_t movesBefore = c->bufMoves.load(std::memory_order_relaxed);
    if (movesBefore != sg->moves) {                                           // (the reservation moved a buffer the other graphs hold)
        if ((s = singleCheckMoves(c, sg)) != GF_OK) return s;
    }
    // once outside a capture: the lean launches use builds of the kernels (1,024 threads) that the batch path of this shape may
    // never have touched -- their code objects are loaded and their LDS attributes set here, not inside the capture
    if ((s = sequence()) != GF_OK) return s;
    GF_HIP(hipStreamSynchronize(c->stream));
    GF_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    s = sequence();
    const hipError_t e2 = hipStreamEndCapture(c->stream, &want.graph);
    const bool moved = c->bufMoves.load(std::memory_order_relaxed) != movesBefore;   // (a capture must not allocate; if it did, its addresses are void)
    if (s != GF_OK || e2 != hipSuccess || !want.graph || moved ||
        hipGraphInstantiate(&want.exec, want.graph, nullptr, nullptr, 0) != hipSuccess) {
        if (want.graph) (void)hipGraphDestroy(want.graph);
        (void)hipGetLastError();
        if (!moved) singleRefused(sg, want.dir * 8 + want.kind, want.nRows, want.nCols, true);   // every later call of this kind: the batch path, directly
        return GF_ERR_UNSUPPORTED;
    }
    sg->graphs.push_back(want);
    *out = &sg->graphs.back();
    return GF_OK;
}

// returns GF_ERR_UNSUPPORTED where the caller should take the batch path instead (first call of a kind, a packing beyond the slot)
static gf_status singleEncode(int kind, gf_context *c, int codecIndex, int nRows, int nCols, const int32_t *values, uint8_t *out,
                              size_t outCap, size_t *outLen, int32_t *tileStatus)
{
    if (!c || nRows < 1 || nCols < 1 || !values || !outLen) return GF_ERR_ARG;
    const size_t cells = (size_t)nRows * (size_t)nCols;
    if (cells * 4 > ((size_t)8 << 20)) return GF_ERR_UNSUPPORTED;            // (large tiles: the batch path's copies are not what they wait for)
    GF_HIP(hipSetDevice(c->device));
    const size_t stride = gf_huffman_default_stride(nRows, nCols);
    gf_status s = singleEnsure(c, std::max(cells * 4, stride + 16), std::max(stride + 64, cells * 4 + 64));
    if (s != GF_OK) return s;
    gf_single *sg = c->single;
    if (singleRefused(sg, kind, nRows, nCols)) return GF_ERR_UNSUPPORTED;
    if (!singleWarmed(sg, kind, nRows, nCols)) return GF_ERR_UNSUPPORTED;
    if ((s = singleCheckMoves(c, sg)) != GF_OK) return s;
    uint8_t *hOut = (uint8_t *)sg->hOut;
    uint32_t *hLen = (uint32_t *)(hOut + stride);
    int32_t *hSt = (int32_t *)(hOut + stride + 4);
    memcpy(sg->hIn, values, cells * 4);
    gf_single_graph *g = nullptr;
    s = singleGraph(c, gf_single_graph{0, kind, nRows, nCols, codecIndex, cells * 4, nullptr, nullptr}, [&]() -> gf_status {
        if (hipMemcpyAsync(sg->dIn.p, sg->hIn, cells * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) return GF_ERR_HIP;
        return encodeBatchDev(kind, c, c->stream, codecIndex, nRows, nCols, 1, (const int32_t *)sg->dIn.p, hOut, stride, hLen, nullptr,
                              hSt, GF_PM_ALL, 1);
    }, &g);
    if (s != GF_OK) return s;
    GF_HIP(hipGraphLaunch(g->exec, c->stream));
    if ((s = singleWait(c->stream)) != GF_OK) return s;
    const int32_t st = *hSt;
    const size_t len = *hLen;
    if (st == GF_OVERFLOW || st == GF_K_LEAN_RETRY) return GF_ERR_UNSUPPORTED;   // longer than the slot, or a kernel this launch left out: the batch path
    *tileStatus = st;
    *outLen = st == GF_OK ? len : 0;
    if (st == GF_OK) {
        if (len > outCap) return GF_ERR_CAPACITY;
        memcpy(out, hOut, len);
    }
    return GF_OK;
}

static gf_status singleDecode(int kind, gf_context *c, int nRows, int nCols, const uint8_t *packing, size_t len, int32_t *values,
                              int32_t *tileStatus)
{
    if (!c || nRows < 1 || nCols < 1 || !packing || !values) return GF_ERR_ARG;
    const size_t cells = (size_t)nRows * (size_t)nCols;
    if (cells * 4 > ((size_t)8 << 20)) return GF_ERR_UNSUPPORTED;
    GF_HIP(hipSetDevice(c->device));
    const size_t stride = gf_huffman_default_stride(nRows, nCols);
    if (len + 16 > stride) return GF_ERR_UNSUPPORTED;                         // (an unusually long packing: the batch path)
    gf_status s = singleEnsure(c, std::max(cells * 4, stride + 16), std::max(stride + 64, cells * 4 + 64));
    if (s != GF_OK) return s;
    gf_single *sg = c->single;
    if (singleRefused(sg, 8 + kind, nRows, nCols)) return GF_ERR_UNSUPPORTED;
    if (!singleWarmed(sg, 8 + kind, nRows, nCols)) return GF_ERR_UNSUPPORTED;
    if ((s = singleCheckMoves(c, sg)) != GF_OK) return s;
    // the copy moves [length, 12 spare bytes, packing]: sized in powers of two so that a few graphs serve every length
    size_t copyBytes = 4096;
    while (copyBytes < len + 16 + 8) copyBytes <<= 1;                         // (+ 8: the kernels read whole words behind the last byte)
    copyBytes = std::min(copyBytes, roundUp(stride + 16, 16));
    uint8_t *hIn = (uint8_t *)sg->hIn, *hOut = (uint8_t *)sg->hOut, *dIn = (uint8_t *)sg->dIn.p;
    int32_t *hSt = (int32_t *)(hOut + cells * 4);
    const uint32_t len32 = (uint32_t)len;
    memcpy(hIn, &len32, 4);
    memcpy(hIn + 16, packing, len);
    memset(hIn + 16 + len, 0, std::min<size_t>(8, copyBytes - 16 - len));
    gf_single_graph *g = nullptr;
    s = singleGraph(c, gf_single_graph{1, kind, nRows, nCols, 0, copyBytes, nullptr, nullptr}, [&]() -> gf_status {
        if (hipMemcpyAsync(dIn, hIn, copyBytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) return GF_ERR_HIP;
        return decodeBatchDev(kind, c, c->stream, nRows, nCols, 1, dIn + 16, copyBytes - 16, nullptr, copyBytes - 16, (const uint32_t *)dIn,
                              (int32_t *)hOut, hSt, 1);
    }, &g);
    if (s != GF_OK) return s;
    GF_HIP(hipGraphLaunch(g->exec, c->stream));
    if ((s = singleWait(c->stream)) != GF_OK) return s;
    if (*hSt == GF_K_LEAN_RETRY) return GF_ERR_UNSUPPORTED;                   // a tile the fast kernel leaves to the others: the batch path
    *tileStatus = *hSt;
    if (*hSt == GF_OK) memcpy(values, hOut, cells * 4);
    return GF_OK;
}

// ICompressionEncoder.encode / ICompressionDecoder.decode: the graph path, else the batch path with one tile (oneTileEncode /
// oneTileDecode have the folding of the tile's status).  The caller holds the context's lock.
static gf_status oneTileEncodeGraph(int kind, gf_context *c, int codecIndex, int nRows, int nCols, const int32_t *values, uint8_t *out,
                                    size_t outCap, size_t *outLen)
{
    if (!outLen) return GF_ERR_ARG;
    int32_t st = 0;
    const gf_status s = singleEncode(kind, c, codecIndex, nRows, nCols, values, out, outCap, outLen, &st);
    if (s == GF_OK) return (gf_status)st;
    if (s != GF_ERR_UNSUPPORTED) return s;
    return oneTileEncode(outLen, [&](uint64_t *offsets, int32_t *tileSt) {
        return encodeBatchHost(kind, c, codecIndex, nRows, nCols, 1, values, out, outCap, offsets, nullptr, tileSt);
    });
}
static gf_status oneTileDecodeGraph(int kind, gf_context *c, int nRows, int nCols, const uint8_t *packing, size_t len, int32_t *values)
{
    int32_t st = 0;
    const gf_status s = singleDecode(kind, c, nRows, nCols, packing, len, values, &st);
    if (s == GF_OK) return (gf_status)st;
    if (s != GF_ERR_UNSUPPORTED) return s;
    return oneTileDecode(len, [&](const uint64_t *offsets, int32_t *tileSt) {
        return decodeBatchHost(kind, c, nRows, nCols, 1, packing, offsets, values, tileSt);
    });
}

extern "C" {

gf_status gf_huffman_encode_batch_i32(gf_context *c, int codecIndex, int nRows, int nCols, size_t nTiles, const int32_t *values,
                                      uint8_t *blob, size_t blobCap, uint64_t *offsets, uint8_t *predictors, int32_t *status)
{
    GF_CTX_LOCK(c);
    return encodeBatchHost(KIND_HUFFMAN, c, codecIndex, nRows, nCols, nTiles, values, blob, blobCap, offsets, predictors, status);
}

gf_status gf_huffman_decode_batch_i32(gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob,
                                      const uint64_t *offsets, int32_t *values, int32_t *status)
{
    GF_CTX_LOCK(c);
    return decodeBatchHost(KIND_HUFFMAN, c, nRows, nCols, nTiles, blob, offsets, values, status);
}

gf_status gf_canon_encode_batch_i32(gf_context *c, int codecIndex, int nRows, int nCols, size_t nTiles, const int32_t *values,
                                    uint8_t *blob, size_t blobCap, uint64_t *offsets, uint8_t *predictors, int32_t *status)
{
    GF_CTX_LOCK(c);
    return encodeBatchHost(KIND_CANON, c, codecIndex, nRows, nCols, nTiles, values, blob, blobCap, offsets, predictors, status);
}

gf_status gf_canon_decode_batch_i32(gf_context *c, int nRows, int nCols, size_t nTiles, const uint8_t *blob,
                                    const uint64_t *offsets, int32_t *values, int32_t *status)
{
    GF_CTX_LOCK(c);
    return decodeBatchHost(KIND_CANON, c, nRows, nCols, nTiles, blob, offsets, values, status);
}

gf_status gf_canon_encode_i32(gf_context *c, int codecIndex, int nRows, int nCols, const int32_t *values, uint8_t *out,
                              size_t outCap, size_t *outLen)
{
    GF_CTX_LOCK(c);
    return oneTileEncodeGraph(KIND_CANON, c, codecIndex, nRows, nCols, values, out, outCap, outLen);
}

gf_status gf_canon_decode_i32(gf_context *c, int nRows, int nCols, const uint8_t *packing, size_t len, int32_t *values)
{
    GF_CTX_LOCK(c);
    return oneTileDecodeGraph(KIND_CANON, c, nRows, nCols, packing, len, values);
}

gf_status gf_huffman_encode_i32(gf_context *c, int codecIndex, int nRows, int nCols, const int32_t *values,
                                uint8_t *out, size_t outCap, size_t *outLen)
{
    GF_CTX_LOCK(c);
    return oneTileEncodeGraph(KIND_HUFFMAN, c, codecIndex, nRows, nCols, values, out, outCap, outLen);
}

gf_status gf_huffman_decode_i32(gf_context *c, int nRows, int nCols, const uint8_t *packing, size_t len,
                                int32_t *values)
{
    GF_CTX_LOCK(c);
    return oneTileDecodeGraph(KIND_HUFFMAN, c, nRows, nCols, packing, len, values);
}

}  // extern "C"
