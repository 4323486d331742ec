// gvrs_file_inspect.hip -- a GVRS file image INSPECTED in device memory: every record walked from the first byte of content and
// checksummed, as GvrsInspector walks a file.  gvrs_file_inspect.h is the host's twin (its header has the reference's lines, the
// order of the checks and the deviations) and shares the judgement of one record's head, gfInspectStepWords, with the kernels here.
// A record's position is the previous record's position plus its size: one lane walking 12,960 records pays a dependent load that
// misses to HBM for every one of them.  So the walk is cut at ANCHORS, record starts known without walking:
//   k_inspect_anchors   a lane per tile directory entry (its position through the place rule before it is touched, then the record's
//                       type and tile index, not its size): atomicMin of position - 8 into the slot of the position's segment.
//                       Segment 0's anchor is the content position; the header's three directory positions are anchors too.
//   k_inspect_walk      a lane per ANCHORED segment walks from its anchor until it reaches or passes the anchor of a later
//                       segment, or stops.  A segment may have no anchor (a long free node spans it) and its anchor need not be
//                       its first record (records the directory does not name stand in front): nothing relies on either.
//   k_inspect_chain     ONE workgroup.  THE CHAIN FROM THE CONTENT POSITION IS THE AUTHORITY: a segment's walk counts only if the
//                       walk in front of it landed exactly on its anchor.  The first anchored segment whose walk did not end on
//                       an anchor ends the chain of walks; a scan over the counts in front of it gives every segment on the chain
//                       its first record's number.  Where that walk passed an anchor without landing on it -- a damaged size
//                       word, an entry that leads into the middle of a record -- lane 0 walks the REST of the image from the
//                       landing point: slow and correct, for damaged files only.  Then the record count against the room and
//                       the head of the record at the header's tile directory position.
//   k_inspect_list      a lane per segment on the chain walks it again and writes its records into the list
//   k_inspect_crc       a wave per record, grid-stride over the list: up to GF_INSPECT_WAVE_CHUNKS chunks by the wave itself (the
//                       scheme of k_record_crc32c_elems), a free node's 8 head bytes and last word and nothing between; a larger
//                       record is handed on
//   k_inspect_crc_large a wave per chunk of GF_INSPECT_CRC_CHUNK bytes of the large records, each chunk's checksum weighed by
//                       x^(8 * bytes behind it) and summed into the record's word (XOR: the order does not matter).  The powers
//                       of x come from tables the compiler makes (gvrs_file_inspect.h): no lane squares and multiplies
//   k_inspect_fold      ONE workgroup: the sequential verdict from the per-record results -- the first record that fails directly
//                       behind a failing one against the structural stop, the counts, the bad tiles compacted in file order by
//                       ballots and a scan, the report
// No byte at or behind the image's length is read: gfInspectStepWords judges a position before it touches it, and a record that
// is checksummed has passed TRUNCATED.  Every launch is sized from the arguments; what depends on the record count is grid-stride
// over the count in GfInspectState.  Plain vector stores only.

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_crc32c.h"
#include "gvrs_file_inspect.h"

namespace {

constexpr uint32_t INS_THREADS = 1024, INS_WAVES = INS_THREADS / 64;

__device__ __forceinline__ void ins_put_anchor(const GfInspectArgs &a, uint64_t q)        // q in [contentPos, bytes)
{
    const uint64_t s = (q - a.p.contentPos) / a.segBytes;
    if (s < a.nSeg) atomicMin(reinterpret_cast<unsigned long long *>(a.anchor + s), (unsigned long long)q);
}

__global__ __launch_bounds__(256) void k_inspect_anchors(const GfInspectArgs a)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x, bytes = a.p.bytes;
    if (k == 0) {
        ins_put_anchor(a, a.p.contentPos);                        // (the smallest position there is: segment 0's anchor)
        const uint64_t dirs[3] = {a.p.tileDirPos, a.metaDirPos, a.freeDirPos};
        for (int i = 0; i < 3; i++)
            if (dirs[i] != 0 && gfRecordPlace(a.p.contentPos, bytes, dirs[i], 0) == GF_PLACE_OK) ins_put_anchor(a, dirs[i] - 8u);
    }
    if (k >= (uint64_t)a.dir.nRows * (uint64_t)a.dir.nCols) return;
    // (gfDirEntryPos and gfRecordPlace written out as before they were shared: with them the sound image measured 0.5 to 1 % slower)
    const uint64_t w = a.dir.extended ? 8u : 4u, at = a.dir.entriesPos + k * w;
    if (at > bytes || w > bytes - at) return;
    const uint64_t p = a.dir.extended ? *reinterpret_cast<const uint64_t *>(a.image + at) : (uint64_t) * reinterpret_cast<const uint32_t *>(a.image + at) * 8u;
    if (p == 0 || p < a.p.contentPos + 8u || (p & 7u) != 0u || p > bytes || bytes - p < 12u) return;
    const uint32_t *h = reinterpret_cast<const uint32_t *>(a.image + (p - 8u));          // (size, type, tile index: ends at p + 4)
    if ((h[1] & 0xffu) != (uint32_t)GF_FILE_REC_TILE || (int32_t)h[2] != gfDirTileOfEntry(a.dir, k)) return;
    ins_put_anchor(a, p - 8u);
}

__global__ __launch_bounds__(256) void k_inspect_walk(const GfInspectArgs a)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= a.nSeg) return;
    uint64_t pos = a.anchor[s];
    if (pos == GF_INSPECT_NONE) return;
    uint32_t cnt = 0, t = s + 1u;
    int code;
    for (;;) {
        gf_file_record r;
        code = gfInspectStepWords(a.p, pos, r, GfLoadAligned{a.image});
        if (code != GF_INSPECT_NEXT) {
            if (code != GF_INSPECT_END) cnt++;
            break;
        }
        cnt++;
        pos += r.size;
        // has the walk reached the anchor of a later segment?  (t: the first later segment not yet known to be without one in front of pos)
        const uint64_t sp = min((pos - a.p.contentPos) / a.segBytes, (uint64_t)a.nSeg - 1u);
        bool hit = false;
        while (t <= sp) {
            const uint64_t q = a.anchor[t];
            if (q == GF_INSPECT_NONE) {
                t++;
                continue;
            }
            if (q <= pos) hit = true, code = q == pos ? GF_INSPECT_LINK : GF_INSPECT_OVERSHOOT;
            break;
        }
        if (hit) break;
    }
    a.landing[s] = pos;
    a.count[s] = cnt;
    a.stopc[s] = code;
}

// the workgroup's exclusive prefix sums of v, and the total in every thread
__device__ __forceinline__ uint64_t ins_block_scan(uint64_t v, uint64_t *waveTot, uint64_t &total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t up = __shfl_up(incl, o, 64);
        if ((int)lane >= o) incl += up;
    }
    __syncthreads();                                              // (waveTot of the round before has been read)
    if (lane == 63u) waveTot[wave] = incl;
    __syncthreads();
    uint64_t before = 0;
    total = 0;
    for (uint32_t k = 0; k < INS_WAVES; k++) {
        if (k < wave) before += waveTot[k];
        total += waveTot[k];
    }
    return before + incl - v;
}

__global__ __launch_bounds__(INS_THREADS) void k_inspect_chain(const GfInspectArgs a)
{
    __shared__ uint32_t first;
    __shared__ uint64_t waveTot[INS_WAVES];
    const uint32_t tid = threadIdx.x;
    if (tid == 0) first = a.nSeg - 1u;
    __syncthreads();
    // the first anchored segment whose walk did not end on an anchor (the last anchored segment is one: nothing lies behind it)
    for (uint32_t s = tid; s < a.nSeg; s += INS_THREADS)
        if (a.anchor[s] != GF_INSPECT_NONE && a.stopc[s] != GF_INSPECT_LINK) atomicMin(&first, s);
    __syncthreads();
    const uint32_t F = first;
    uint64_t running = 0;
    for (uint32_t s0 = 0; s0 <= F; s0 += INS_THREADS) {
        const uint32_t s = s0 + tid;
        const bool on = s <= F && a.anchor[s] != GF_INSPECT_NONE;
        uint64_t total;
        const uint64_t before = ins_block_scan(on ? a.count[s] : 0u, waveTot, total);
        if (s <= F) a.base[s] = on ? running + before : GF_INSPECT_NONE;
        running += total;
    }
    for (uint32_t s = F + 1u + tid; s < a.nSeg; s += INS_THREADS) a.base[s] = GF_INSPECT_NONE;
    if (tid != 0) return;
    const bool anchored = a.anchor[F] != GF_INSPECT_NONE;         // (always: segment 0 is, and the last anchored segment's walk ends on none)
    uint64_t n = running, pos = anchored ? a.landing[F] : a.p.contentPos;
    int code = anchored ? a.stopc[F] : GF_INSPECT_OVERSHOOT;
    if (code == GF_INSPECT_OVERSHOOT) {                           // the link did not close: the rest of the image, serially
        for (;;) {
            gf_file_record r;
            code = gfInspectStepWords(a.p, pos, r, GfLoadAligned{a.image});
            if (code == GF_INSPECT_END) break;
            if (n < a.maxRecords) a.recs[n] = r;
            n++;
            if (code != GF_INSPECT_NEXT) break;
            pos += r.size;
        }
    }
    GfInspectState st{};
    st.status = n > a.maxRecords ? GF_K_ERR_CAPACITY : GF_K_OK;
    st.stop = code, st.n = n, st.term = pos;
    *a.state = st;
    // the record at the header's tile directory position: judged here, checksummed with the others
    gf_file_record d{};
    const uint64_t T = a.p.tileDirPos;
    if (gfRecordPlace(a.p.contentPos, a.p.bytes, T, 0) == GF_PLACE_OK) {
        const uint32_t *h = reinterpret_cast<const uint32_t *>(a.image + (T - 8u));
        if (gfInspectDirHead(a.p, T, h[0], h[1])) d.pos = T - 8u, d.size = h[0], d.type = -1, d.checksum = -1;
    }
    a.recs[a.maxRecords] = d;                                     // (size 0: refused, the checksum failed)
}

__global__ __launch_bounds__(256) void k_inspect_list(const GfInspectArgs a)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= a.nSeg || a.state->status != GF_K_OK) return;
    const uint64_t b = a.base[s];
    if (b == GF_INSPECT_NONE) return;
    uint64_t pos = a.anchor[s];
    const uint32_t cnt = a.count[s];
    for (uint32_t i = 0; i < cnt; i++) {
        gf_file_record r;
        (void)gfInspectStepWords(a.p, pos, r, GfLoadAligned{a.image});
        a.recs[b + i] = r;
        pos += r.size;
    }
}

// the powers of x (gvrs_file_inspect.h), made by the compiler: read through the cache, 4 KB and a few words
__device__ const GfInspectPowers INS_POW = gfInspectMakePowers();

// the CRC-32C of r[0, nBytes) by the whole wave, nBytes a multiple of 4 of at most GF_INSPECT_WAVE_CHUNKS chunks and r 8-byte
// aligned: lane l takes the l-th of 64 runs (a multiple of 16 bytes each) of the whole 16-byte pieces, the runs are joined as
// gvrs_crc32c.h says with powers from the table, and the up to 12 bytes behind them are run through the byte table by every
// lane.  Every lane returns the checksum.  (Its own split, not wave_crc_bytes: the runs end on the table's powers.)
__device__ __forceinline__ uint32_t ins_wave_crc(const uint32_t *table, const uint8_t *r, uint32_t nBytes, uint32_t lane)
{
    const uint32_t nFull = nBytes & ~15u, per = ((nFull / 16u + 63u) / 64u) * 16u;
    const uint32_t begin = min(nFull, lane * per), end = min(nFull, begin + per);
    uint32_t at = begin;
    __builtin_assume(((end - begin) & 15u) == 0u);                // (whole pieces only)
    const uint32_t crc = ~crc_pieces16(table, 0xffffffffu, r, at, end);   // the run's own checksum (an empty run: 0)
    uint32_t part = wave_xor(gfCrcMulmod(INS_POW.small[(nFull - end) / 16u], crc));
    part ^= 0xffffffffu;                                          // the checksum of the whole pieces goes on over the rest
    for (uint32_t i = nFull; i < nBytes; i += 4u) part = crc_word(table, part, *reinterpret_cast<const uint32_t *>(r + i));
    return part ^ 0xffffffffu;
}

// a large record's bytes in front of its checksum: all of them, and the whole 16-byte pieces k_inspect_crc_large takes
__device__ __forceinline__ uint32_t ins_large_whole(uint32_t nBytes) { return nBytes & ~15u; }

// is record w of the work list checksummed, and over how many bytes?  The work list: the records of the walk where the file has
// checksums, then the record at the tile directory position.  A structural stop's record is not checksummed.
__device__ __forceinline__ bool ins_crc_work(const GfInspectArgs &a, const GfInspectState &st, uint64_t w, uint64_t &idx, gf_file_record &r, uint32_t &nBytes)
{
    const uint64_t nWalk = a.p.checksums ? st.n : 0u;
    idx = w < nWalk ? w : a.maxRecords;
    r = a.recs[idx];
    if (w < nWalk) {
        if (st.stop != GF_INSPECT_END && w == st.n - 1u) return false;
        nBytes = r.type == GF_FILE_REC_FREE ? 8u : r.size - 4u;
        return true;
    }
    nBytes = r.size - 4u;
    return r.size != 0u;
}

__global__ __launch_bounds__(256) void k_inspect_crc(const GfInspectArgs a)
{
    __shared__ uint32_t table[256];
    crc_table_fill_256(table);
    const GfInspectState st = *a.state;
    if (st.status != GF_K_OK) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nWork = (a.p.checksums ? st.n : 0u) + 1u;
    for (uint64_t w = (uint64_t)blockIdx.x * 4u + gf_wave_id(); w < nWork; w += (uint64_t)gridDim.x * 4u) {
        uint64_t idx;
        gf_file_record r;
        uint32_t nBytes;
        if (!ins_crc_work(a, st, w, idx, r, nBytes)) continue;
        if (nBytes > GF_INSPECT_WAVE_CHUNKS * GF_INSPECT_CRC_CHUNK) {
            if (lane == 0u) {
                a.large[atomicAdd(&a.state->nLarge, 1u)] = (uint32_t)idx;
                a.recs[idx].checksum = 2;                         // (k_inspect_fold settles it)
            }
            continue;
        }
        const uint8_t *p = a.image + r.pos;
        const uint32_t crc = ins_wave_crc(table, p, nBytes, lane);
        if (lane == 0u) a.recs[idx].checksum = crc == *reinterpret_cast<const uint32_t *>(p + r.size - 4u) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_inspect_crc_large(const GfInspectArgs a)
{
    __shared__ uint32_t table[256];
    crc_table_fill_256(table);
    const GfInspectState st = *a.state;
    if (st.status != GF_K_OK) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nWaves = (uint64_t)gridDim.x * 4u, wave = (uint64_t)blockIdx.x * 4u + gf_wave_id();
    for (uint32_t k = 0; k < st.nLarge; k++) {
        const uint32_t idx = a.large[k];
        const gf_file_record r = a.recs[idx];
        const uint32_t nWhole = ins_large_whole(r.size - 4u), nChunks = (nWhole + GF_INSPECT_CRC_CHUNK - 1u) / GF_INSPECT_CRC_CHUNK;
        for (uint64_t c = (wave + k) % nWaves; c < nChunks; c += nWaves) {        // (+ k: the records' first chunks do not all fall to wave 0)
            const uint32_t at = (uint32_t)c * GF_INSPECT_CRC_CHUNK, len = min(GF_INSPECT_CRC_CHUNK, nWhole - at);
            uint32_t crc = ins_wave_crc(table, a.image + r.pos + at, len, lane);
            // its weight x^(8 * bytes behind it): the product of the table's powers over the set bits of the distance in 16-byte pieces
            for (uint32_t e = (nWhole - at - len) / 16u, i = 0; e; e >>= 1, i++)
                if (e & 1u) crc = gfCrcMulmod(INS_POW.two[i], crc);
            if (lane == 0u) atomicXor(a.acc + idx, crc);
        }
    }
}

__global__ __launch_bounds__(INS_THREADS) void k_inspect_fold(const GfInspectArgs a)
{
    __shared__ unsigned long long firstDouble, byType[7], nFail;
    __shared__ uint32_t dirPassed, waveCnt[INS_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const GfInspectState st = *a.state;
    gf_file_inspect_report o{};
    if (st.status != GF_K_OK) {
        if (tid == 0) {
            o.status = GF_K_ERR_CAPACITY, o.n_records = st.n;
            *a.report = o;
        }
        return;
    }
    if (tid == 0) firstDouble = GF_INSPECT_NONE, nFail = 0, dirPassed = 0;
    if (tid < 7) byType[tid] = 0;
    // the large records' checksums against their last words
    for (uint32_t k = tid; k < st.nLarge; k += INS_THREADS) {
        const uint32_t idx = a.large[k];
        const gf_file_record r = a.recs[idx];
        uint32_t crc = ~a.acc[idx];                               // (the whole pieces' checksum goes on over the up to 12 bytes behind them)
        for (uint32_t i = ins_large_whole(r.size - 4u); i < r.size - 4u; i += 4u)
            crc = gfCrcWordBits(crc, *reinterpret_cast<const uint32_t *>(a.image + r.pos + i));
        a.recs[idx].checksum = ~crc == *reinterpret_cast<const uint32_t *>(a.image + r.pos + r.size - 4u) ? 1 : 0;
    }
    __syncthreads();
    // the first record that fails directly behind a failing one (a structural stop's record has no checksum: it is never one)
    for (uint64_t i = 1u + tid; i < st.n; i += INS_THREADS)
        if (a.recs[i].checksum == 0 && a.recs[i - 1u].checksum == 0) {
            atomicMin(&firstDouble, (unsigned long long)i);
            break;                                                // (this thread's later records are behind it)
        }
    __syncthreads();
    const bool twice = firstDouble != GF_INSPECT_NONE;
    const uint64_t n = twice ? firstDouble + 1u : st.n;
    const int stop = twice ? GF_INSPECT_TWO_CHECKSUM_FAILURES : st.stop;
    uint64_t nBad = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += INS_THREADS) {
        const uint64_t i = i0 + tid;
        bool bad = false;
        int32_t tile = 0;
        if (i < n) {
            const gf_file_record r = a.recs[i];
            if (a.records) a.records[i] = r;
            if (r.type >= 0 && r.type <= 6) atomicAdd(&byType[r.type], 1ull);
            if (r.checksum == 0) atomicAdd(&nFail, 1ull);
            if (r.checksum == 1 && r.type == GF_FILE_REC_TILE_DIR) dirPassed = 1u;
            bad = (r.checksum == 0 && r.type == GF_FILE_REC_TILE) || (stop == GF_INSPECT_TILE_TOO_LARGE && i == n - 1u);
            tile = r.tile_index;
        }
        // the bad tiles in file order: the rank among the wave's lanes by ballot, the waves in front by their counts
        const uint64_t m = __ballot(bad);
        const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        __syncthreads();                                          // (waveCnt of the round before has been read)
        if (lane == 0u) waveCnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint64_t before = 0, total = 0;
        for (uint32_t k = 0; k < INS_WAVES; k++) {
            if (k < wave) before += waveCnt[k];
            total += waveCnt[k];
        }
        if (bad && nBad + before + rank < a.badCap) a.badTiles[nBad + before + rank] = tile;
        nBad += total;
    }
    __syncthreads();
    if (tid != 0) return;
    o.status = GF_K_OK;
    o.stop = stop;
    o.complete = stop == GF_INSPECT_END;
    o.failed = stop != GF_INSPECT_END || nFail != 0;
    o.bad_tile_index = stop == GF_INSPECT_BAD_TILE_INDEX, o.invalid_record_size = stop == GF_INSPECT_TILE_TOO_LARGE;
    o.tile_dir_located = 1;
    o.tile_dir_passed = a.recs[a.maxRecords].checksum == 1 || dirPassed != 0u;
    o.termination_pos = twice ? a.recs[n - 1u].pos : st.term;
    o.n_records = n, o.n_checksum_failures = nFail, o.n_bad_tiles = nBad;
    for (int k = 0; k < 7; k++) o.n_by_type[k] = byType[k];
    *a.report = o;
}

}  // namespace

#ifdef GF_DIAG
// the diagnostic flavour only (tools/file_inspect_rate.py): an event in front of every kernel and behind the last, so that the time
// splits by kernel; gf_internal_inspect_kernel_ms waits for the last one
static hipEvent_t g_insEvents[8];
static bool g_insTimed = false, g_insMade = false;
extern "C" void gf_internal_inspect_time_kernels(int on)
{
    if (on && !g_insMade) {
        for (hipEvent_t &e : g_insEvents) (void)hipEventCreate(&e);
        g_insMade = true;
    }
    g_insTimed = on != 0;
}
extern "C" int gf_internal_inspect_kernel_ms(float ms[7])
{
    if (!g_insMade || hipEventSynchronize(g_insEvents[7]) != hipSuccess) return -1;
    for (int k = 0; k < 7; k++)
        if (hipEventElapsedTime(ms + k, g_insEvents[k], g_insEvents[k + 1]) != hipSuccess) return -1;
    return 0;
}
#define INS_MARK(k) do { if (g_insTimed) (void)hipEventRecord(g_insEvents[k], stream); } while (0)
#else
#define INS_MARK(k) do { } while (0)
#endif

hipError_t gf_launch_file_inspect(const GfInspectArgs &a, hipStream_t stream)
{
    const uint64_t nEntries = (uint64_t)a.dir.nRows * (uint64_t)a.dir.nCols;
    if (a.nSeg < 1u || a.segBytes < 8u || a.dir.nRows < 0 || a.dir.nCols < 0 || nEntries > 0x7fffffffull || a.dir.nColsOfTiles < 1) return hipErrorInvalidValue;
    if (((uintptr_t)a.image & 7u) != 0 || !gfDirEntriesAligned(a.dir) || (a.p.contentPos & 7u) != 0 || a.maxRecords > 0x7ffffffeull) return hipErrorInvalidValue;
    const unsigned segBlocks = (a.nSeg + 255u) / 256u;
    const unsigned crcBlocks = (unsigned)std::min<uint64_t>((a.maxRecords + 1u + 3u) / 4u, 8192u);
    INS_MARK(0);
    hipLaunchKernelGGL(k_inspect_anchors, dim3((unsigned)(std::max<uint64_t>(nEntries, 1u) + 255u) / 256u), dim3(256), 0, stream, a);
    INS_MARK(1);
    hipLaunchKernelGGL(k_inspect_walk, dim3(segBlocks), dim3(256), 0, stream, a);
    INS_MARK(2);
    hipLaunchKernelGGL(k_inspect_chain, dim3(1), dim3(INS_THREADS), 0, stream, a);
    INS_MARK(3);
    hipLaunchKernelGGL(k_inspect_list, dim3(segBlocks), dim3(256), 0, stream, a);
    INS_MARK(4);
    hipLaunchKernelGGL(k_inspect_crc, dim3(crcBlocks), dim3(256), 0, stream, a);
    INS_MARK(5);
    hipLaunchKernelGGL(k_inspect_crc_large, dim3(256), dim3(256), 0, stream, a);
    INS_MARK(6);
    hipLaunchKernelGGL(k_inspect_fold, dim3(1), dim3(INS_THREADS), 0, stream, a);
    INS_MARK(7);
    return hipGetLastError();
}
