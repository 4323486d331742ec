// gvrs_api.hip -- the C ABI of include/gvrs_hip_codec.h: version, status strings and the last error, the context, strides, the
// device and host memory helpers and the timers.  The codecs are in the other gvrs_api_*.hip (host paths: which file holds what).
// No CPU fallback anywhere: every compute call needs a HIP device.

#include "gvrs_api_internal.h"

thread_local std::string g_lastError;
#ifdef GF_DIAG
int g_encPhaseLimit = 0, g_decPhaseLimit = 0;
uint32_t *g_decodeDebug = nullptr;   // 16 cycle stamps per tile
uint32_t *g_encodeDebug = nullptr;   // dump target of the next encode launches
#endif

struct gf_timer {
    gf_context *ctx;
    hipEvent_t start, stop;
};

// Cores this process may really use: the affinity mask capped by the cgroup CPU quota (a container that shows 256 CPUs may
// be allowed 16 cores' worth of time; more threads than that only take turns and thrash the caches).
unsigned hostCores()
{
    static const unsigned cached = []() -> unsigned {
        unsigned n = std::thread::hardware_concurrency();
        if (n == 0) n = 1;
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::min<unsigned>(n, (unsigned)std::max(1, CPU_COUNT(&set)));
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {                       // cgroup v2: "<quota|max> <period>"
            char q[64];
            long long period = 0;
            if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0)
                n = std::min<unsigned>(n, (unsigned)std::max<long long>(1, atoll(q) / period));
            fclose(f);
        } else if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {   // cgroup v1
            long long quota = -1, period = 0;
            if (fscanf(g, "%lld", &quota) != 1) quota = -1;
            fclose(g);
            if (FILE *h = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
                if (fscanf(h, "%lld", &period) != 1) period = 0;
                fclose(h);
            }
            if (quota > 0 && period > 0) n = std::min<unsigned>(n, (unsigned)std::max<long long>(1, quota / period));
        }
        return std::min(n, 256u);
    }();
    return cached;
}

extern "C" {

const char *gf_version(void) { return "gvrs-hip-codec 0.1 (gfx950)"; }

#ifdef GF_DIAG
// Not part of the public ABI (diagnostic flavour only): lets tools/ capture the encode kernel's on-chip tables
// (gvrs_encode_layout.h).  d_words must hold gf_internal_encode_debug_words() uint32 per tile.
void gf_internal_set_encode_debug(void *d_words) { g_encodeDebug = (uint32_t *)d_words; }
void gf_internal_set_decode_debug(void *d_words) { g_decodeDebug = (uint32_t *)d_words; }
void gf_internal_set_phase_limits(int enc, int dec) { g_encPhaseLimit = enc; g_decPhaseLimit = dec; }
size_t gf_internal_encode_debug_words(void) { return GF_ENC_DEBUG_WORDS; }
#endif

const char *gf_status_string(int s)
{
    switch (s) {
    case GF_OK: return "ok";
    case GF_DECLINED: return "declined (encoder returns null)";
    case GF_OVERFLOW: return "packing larger than the output slot";
    case GF_ERR_FORMAT: return "format error (IOException in the reference)";
    case GF_ERR_BOUNDS: return "out of bounds (ArrayIndexOutOfBounds in the reference)";
    case GF_ERR_CAPACITY: return "output buffer too small";
    case GF_ERR_ARG: return "bad argument";
    case GF_ERR_NO_DEVICE: return "no HIP device";
    case GF_ERR_HIP: return "HIP runtime error";
    case GF_ERR_UNSUPPORTED: return "unsupported";
    default: return "unknown status";
    }
}

const char *gf_last_error(void) { return g_lastError.c_str(); }
// (library-internal: gvrs_multi.hip hands the text of a failing shard's thread to the thread that called gf_*_multi)
// (an internal hook of gvrs_multi.hip, not part of the ABI: hidden from the library's exports)
__attribute__((visibility("hidden"))) void gf_internal_set_last_error(const char *text) { g_lastError = text ? text : ""; }

int gf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

gf_status gf_context_create(int device, gf_context **out)
{
    if (!out) return GF_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        g_lastError = "no HIP device visible";
        return GF_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) return GF_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return GF_ERR_NO_DEVICE;
    gf_context *c = new (std::nothrow) gf_context();
    if (!c) return GF_ERR_ARG;
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        hipFail(e, "hipStreamCreate");
        return GF_ERR_NO_DEVICE;
    }
    gf_status s = c->flags.ensure(64);
    if (s != GF_OK) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return s;
    }
    // (words 2 and 3 -- count and cursor of the roomy decode run's tile list -- start at zero; the kernels leave them so)
    if (hipMemset(c->flags.p, 0, 64) != hipSuccess) {
        (void)hipGetLastError();
        c->flags.release();
        (void)hipStreamDestroy(c->stream);
        delete c;
        return GF_ERR_HIP;
    }
    if (hipHostMalloc((void **)&c->hRoomySeen, 64, hipHostMallocDefault) == hipSuccess) *c->hRoomySeen = 0u;
    else { (void)hipGetLastError(); c->hRoomySeen = nullptr; }
    // (the side stream is an optimisation: without it the roomy run follows the first one on the caller's stream)
    if (hipStreamCreateWithFlags(&c->side.stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->side.fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->side.join, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        if (c->side.fork) (void)hipEventDestroy(c->side.fork);
        if (c->side.stream) (void)hipStreamDestroy(c->side.stream);
        c->side = GfSideStream{nullptr, nullptr, nullptr};
    }
    *out = c;
    return GF_OK;
}

void gf_context_destroy(gf_context *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    gf_single_destroy(c->single);
    c->single = nullptr;
    for (DevBuf *b = c->bufs; b; b = b->next) b->release();
    gf_host_pipe_destroy(c->pipe);
    c->hRecCounts.release();
    c->hFileFront.release();
    if (c->fileFrontDone) (void)hipEventDestroy(c->fileFrontDone);
    if (c->hRoomySeen) (void)hipHostFree(c->hRoomySeen);
    if (c->side.stream) {
        (void)hipStreamSynchronize(c->side.stream);
        (void)hipEventDestroy(c->side.fork);
        (void)hipEventDestroy(c->side.join);
        (void)hipStreamDestroy(c->side.stream);
    }
    (void)hipStreamDestroy(c->stream);
    delete c;
}

void *gf_context_stream(gf_context *c) { return c ? (void *)c->stream : nullptr; }

gf_status gf_context_synchronize(gf_context *c)
{
    GF_CTX_LOCK(c);
    if (!c) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    GF_HIP(hipStreamSynchronize(c->stream));
    return GF_OK;
}

gf_status gf_context_reserve(gf_context *c, int nRows, int nCols, size_t nTiles)
{
    GF_CTX_LOCK(c);
    if (!c || nRows < 1 || nCols < 1) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    uint64_t need[3];
    scratchReserve(nRows, nCols, nTiles, need);
    gf_status s = c->trees.ensure(need[1]);
    if (s != GF_OK) return s;
    if ((s = c->packRecs.ensure(need[2])) != GF_OK) return s;
    return c->workspace.ensure(need[0]);
}

// Not part of the public ABI (tests load it by name): bytes held of workspace, trees, packRecs and of all the context's buffers; their moves
gf_status gf_internal_context_scratch(gf_context *c, uint64_t out[5])
{
    GF_CTX_LOCK(c);
    if (!c || !out) return GF_ERR_ARG;
    out[0] = c->workspace.bytes, out[1] = c->trees.bytes, out[2] = c->packRecs.bytes, out[3] = 0;
    for (const DevBuf *b = c->bufs; b; b = b->next) out[3] += b->bytes;
    out[4] = c->bufMoves.load(std::memory_order_relaxed);
    return GF_OK;
}

size_t gf_huffman_default_stride(int nRows, int nCols)
{
    return roundUp((size_t)4 * (size_t)nRows * (size_t)nCols + 1024, 16);
}

size_t gf_huffman_max_packing(int nRows, int nCols)
{
    // 80 header bits + tree (8 + 10*256 - 1) + 6 M32 bytes per cell at <= 46 bits per code
    // (depth d needs Fib(d+2) symbols; nM32 < 2^31 bounds d by 44)
    const size_t cells = (size_t)nRows * (size_t)nCols;
    const size_t bits = 80 + 8 + 2559 + cells * 6 * 46;
    return roundUp((bits + 7) / 8 + 16, 16);
}

// ------------------------------------------------------------------ device memory helpers

// page-locked host memory: the host-memory batch entry points move it over PCIe in place (no staging copy)
gf_status gf_host_alloc(size_t bytes, void **p)
{
    if (!p) return GF_ERR_ARG;
    *p = nullptr;
    GF_HIP(hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocPortable));
    return GF_OK;
}

gf_status gf_host_free(void *p)
{
    if (p) GF_HIP(hipHostFree(p));
    return GF_OK;
}

gf_status gf_dev_malloc(gf_context *c, size_t bytes, void **p)
{
    GF_CTX_LOCK(c);
    if (!c || !p) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    GF_HIP(hipMalloc(p, bytes ? bytes : 16));
    return GF_OK;
}

gf_status gf_dev_free(gf_context *c, void *p)
{
    GF_CTX_LOCK(c);
    if (!c) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    GF_HIP(hipFree(p));
    return GF_OK;
}

gf_status gf_dev_memset(gf_context *c, void *p, int value, size_t bytes)
{
    GF_CTX_LOCK(c);
    if (!c) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    GF_HIP(hipMemsetAsync(p, value, bytes, c->stream));
    GF_HIP(hipStreamSynchronize(c->stream));
    return GF_OK;
}

gf_status gf_dev_upload(gf_context *c, void *d, const void *h, size_t bytes)
{
    GF_CTX_LOCK(c);
    if (!c) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    GF_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    GF_HIP(hipStreamSynchronize(c->stream));
    return GF_OK;
}

gf_status gf_dev_download(gf_context *c, void *h, const void *d, size_t bytes)
{
    GF_CTX_LOCK(c);
    if (!c) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));                        // launches and copies below go to the context's device
    GF_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
    GF_HIP(hipStreamSynchronize(c->stream));
    return GF_OK;
}

// ------------------------------------------------------------------ timers

gf_status gf_timer_create(gf_context *c, gf_timer **out)
{
    GF_CTX_LOCK(c);
    if (!c || !out) return GF_ERR_ARG;
    GF_HIP(hipSetDevice(c->device));
    gf_timer *t = new (std::nothrow) gf_timer();
    if (!t) return GF_ERR_ARG;
    t->ctx = c;
    GF_HIP(hipEventCreate(&t->start));
    GF_HIP(hipEventCreate(&t->stop));
    *out = t;
    return GF_OK;
}

void gf_timer_destroy(gf_timer *t)
{
    if (!t) return;
    (void)hipEventDestroy(t->start);
    (void)hipEventDestroy(t->stop);
    delete t;
}

gf_status gf_timer_start(gf_timer *t, void *stream)
{
    if (!t) return GF_ERR_ARG;
    GF_HIP(hipEventRecord(t->start, streamOf(t->ctx, stream)));
    return GF_OK;
}

gf_status gf_timer_stop(gf_timer *t, void *stream)
{
    if (!t) return GF_ERR_ARG;
    GF_HIP(hipEventRecord(t->stop, streamOf(t->ctx, stream)));
    return GF_OK;
}

gf_status gf_timer_elapsed_ms(gf_timer *t, float *ms)
{
    if (!t || !ms) return GF_ERR_ARG;
    GF_HIP(hipEventSynchronize(t->stop));
    GF_HIP(hipEventElapsedTime(ms, t->start, t->stop));
    return GF_OK;
}

}  // extern "C"
