// gvrs_tabulate.hip -- what is in a grid block that lies in device memory: the dense counters, range and sums of the reference's
// InputDataStatCollector / PackageData (k_tabulate_dense, k_tabulate_finish) and the table of distinct 32-bit symbols with their
// counts that its EntropyTabulator keeps in a 16 GB file of counters (a radix sort of the symbols: k_tab_digit_hist,
// k_tab_digit_scan, k_tab_scatter; then k_tab_runs).  The arithmetic is gvrs_tabulate_common.h, shared with the CPU harness; this
// file is the data path.  Every result is integers or a comparison with a definite tie rule: bit-exact whatever the order.
//
// k_tabulate_dense, up to GF_TAB_MAX_GROUPS persistent workgroups of GF_TAB_THREADS lanes striding the block with 16-byte loads
// (4 INT / FLOAT cells, 8 SHORT cells a lane; the cells in front of the first 16-byte boundary and behind the last whole load are
// taken one a lane).  LDS: the counters are private to the workgroup in LDS (n_bins <= GF_TAB_LDS_MAX_BINS) and the non-zero ones
// are flushed once with global atomics; else every sample is one global atomic.  A lane keeps the range and sums of its cells,
// visited in ascending order; they are merged per wave, then per workgroup into the context's partials array, and
// k_tabulate_finish merges those (and, accumulating, what the summary held) into the summary.
//
// The sort is least-significant-digit first with 8-bit digits, keys only, stable: a workgroup owns a contiguous share of the keys,
// k_tab_digit_hist counts its digits into hist[digit][workgroup], k_tab_digit_scan turns that array, flattened, into the exclusive
// scan (three phases: sums of GF_TAB_SCAN_BLOCK entries, one workgroup over the sums, the entries), and k_tab_scatter walks the
// share in rounds of GF_TAB_SORT_THREADS keys, ranking the keys of a round by wave ballots: equal digits keep their input order.
// k_tab_runs: phase 0 counts the run heads of GF_TAB_RUN_BLOCK sorted keys (scanned by k_tab_digit_scan), phase 1 writes every
// head's position and symbol, phase 2 turns positions into counts and adds up the scalars.
//
// Two tables merged (gvrs_tabulate_common.h states the merged sequence and the pair rule): k_tab_merge_splits finds the split of
// every chunk of GF_TAB_MERGE_BLOCK positions by binary search, k_tab_merge merges a chunk in LDS -- phase 0 counts its heads
// (scanned by k_tab_digit_scan), k_tab_merge_head writes the summary, phase 1 writes symbols and summed counts and adds up the
// scalars.  A SHORT block by counters: k_tab_short_counts (a window of the 65,536 counters in LDS, the rest by global atomics),
// k_tab_short_compact (the counters that are not 0, in the symbols' order).
//
// Nothing outside the block is read; the counters, the summary, the tables up to their capacity and the context's temporaries
// are all that is written.

#include <hip/hip_runtime.h>

#include <type_traits>

#include "gvrs_kernels.h"
#include "gvrs_common.h"
#include "gvrs_tabulate_common.h"

namespace {

constexpr uint32_t TAB_WAVES = GF_TAB_THREADS / 64;

// ---------------------------------------------------------------- the dense form

using TabPartD = GfTabPart<double>;

__device__ __forceinline__ TabPartD tabShflDown(const TabPartD &p, int off)
{
    TabPartD q;
    q.nSkipped = __shfl_down((unsigned long long)p.nSkipped, off, 64), q.nSamples = __shfl_down((unsigned long long)p.nSamples, off, 64);
    q.sumSamples = __shfl_down((unsigned long long)p.sumSamples, off, 64), q.sumI = __shfl_down((unsigned long long)p.sumI, off, 64);
    q.mn.v = __shfl_down(p.mn.v, off, 64), q.mn.at = __shfl_down((long long)p.mn.at, off, 64);
    q.mx.v = __shfl_down(p.mx.v, off, 64), q.mx.at = __shfl_down((long long)p.mx.at, off, 64);
    return q;
}

// lane 0 of the wave ends with the wave's part (every lane of the wave takes part)
__device__ __forceinline__ void tabWaveMerge(TabPartD &p)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const TabPartD q = tabShflDown(p, off);
        if ((threadIdx.x & 63) + off < 64) gf_tab_part_merge(p, q);
    }
}

__device__ __forceinline__ void tabToPartial(const TabPartD &p, GfTabPartial &o)
{
    o.nSkipped = p.nSkipped, o.nSamples = p.nSamples, o.sumSamples = p.sumSamples, o.sumI = p.sumI;
    o.mn = p.mn.v, o.mx = p.mx.v, o.mnAt = p.mn.at, o.mxAt = p.mx.at;
}
__device__ __forceinline__ TabPartD tabFromPartial(const GfTabPartial &o)
{
    TabPartD p;
    p.nSkipped = o.nSkipped, p.nSamples = o.nSamples, p.sumSamples = o.sumSamples, p.sumI = o.sumI;
    p.mn.v = o.mn, p.mx.v = o.mx, p.mn.at = o.mnAt, p.mx.at = o.mxAt;
    return p;
}

template <typename T>
__device__ __forceinline__ T tabCellOf(const uint4 &x, int c)
{
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
    if constexpr (sizeof(T) == 2) return (T)(int16_t)(uint16_t)(w[c >> 1] >> (16 * (c & 1)));
    else if constexpr (std::is_floating_point_v<T>) return __uint_as_float(w[c]);
    else return (T)(int32_t)w[c];
}

// head: cells in front of the first 16-byte boundary; nVec: whole 16-byte loads behind them; dynamic LDS: the counters (LDS form),
// then TAB_WAVES parts.  A lane numbers the cells of its loads 0, 1, 2, ... in an int32 (trip * CPV + cell of the load; the
// launcher keeps that below 2^31) and turns the two numbers it kept into global indices behind the loop; its head and tail cells,
// one each at most, go through a part of their own.  UNIT: gf_tab_cell's.
template <typename T, bool LDS, bool UNIT>
__global__ __launch_bounds__(GF_TAB_THREADS) void k_tabulate_dense(const GfTabDenseGeom g, const T *__restrict__ block, int32_t *__restrict__ counter,
                                                                   GfTabPartial *__restrict__ partials, const int64_t head, const int64_t nVec)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t tabLds[];
    constexpr int CPV = 16 / (int)sizeof(T);
    const uint32_t tid = threadIdx.x;
    const uint32_t nBins = (uint32_t)g.nCounter + 1u;
    const uint32_t ldsBins = LDS ? (nBins + 3u) & ~3u : 0u;
    if constexpr (LDS) {
        for (uint32_t i = tid; i < nBins; i += GF_TAB_THREADS) tabLds[i] = 0;
        __syncthreads();
    }
    auto count = [&](int32_t index) {
        if (index < 0) return;
        if constexpr (LDS) atomicAdd(&tabLds[index], 1u);
        else atomicAdd(&counter[index], 1);
    };
    const int64_t gid = (int64_t)blockIdx.x * GF_TAB_THREADS + tid, stride = (int64_t)gridDim.x * GF_TAB_THREADS;
    GfTabPart<T> ends;                                                             // the head cell, then the tail cell
    gf_tab_part_start(ends);
    if (gid < head) count(gf_tab_cell<UNIT>(g, block[gid], g.firstCell + gid, ends));
    GfTabPart<T, int32_t> p;
    gf_tab_part_start(p);
    const uint4 *vec = reinterpret_cast<const uint4 *>(block + head);
    int32_t seq = 0;
    for (int64_t v = gid; v < nVec; v += stride, seq += CPV) {
        const uint4 x = vec[v];
#pragma unroll
        for (int c = 0; c < CPV; c++) count(gf_tab_cell<UNIT>(g, tabCellOf<T>(x, c), seq + c, p));
    }
    // the loads' part with global indices, between the head cell's and the tail cell's
    auto global = [&](int32_t s) { return s < 0 ? (int64_t)-1 : g.firstCell + head + (gid + (int64_t)(s / CPV) * stride) * CPV + s % CPV; };
    GfTabPart<T> q;
    q.nSkipped = p.nSkipped, q.nSamples = p.nSamples, q.sumSamples = p.sumSamples, q.sumI = p.sumI;
    q.mn.v = p.mn.v, q.mn.at = global(p.mn.at), q.mx.v = p.mx.v, q.mx.at = global(p.mx.at);
    gf_tab_part_merge(ends, q);
    const int64_t tail0 = head + nVec * CPV;
    if (gid < g.nCells - tail0) count(gf_tab_cell<UNIT>(g, block[tail0 + gid], g.firstCell + tail0 + gid, ends));

    TabPartD d = gf_tab_widen(ends);
    tabWaveMerge(d);
    GfTabPartial *parts = reinterpret_cast<GfTabPartial *>(tabLds + ldsBins);
    if ((tid & 63) == 0) tabToPartial(d, parts[tid >> 6]);
    __syncthreads();
    if (tid == 0) {
        for (uint32_t w = 1; w < TAB_WAVES; w++) gf_tab_part_merge(d, tabFromPartial(parts[w]));
        tabToPartial(d, partials[blockIdx.x]);
    }
    if constexpr (LDS) {
        for (uint32_t i = tid; i < nBins; i += GF_TAB_THREADS) {
            const uint32_t c = tabLds[i];
            if (c) atomicAdd(&counter[i], (int32_t)c);
        }
    }
}

// one workgroup of GF_TAB_MAX_GROUPS lanes: the partials (nPartials <= GF_TAB_MAX_GROUPS) and, accumulating, the summary as it was
__global__ __launch_bounds__(GF_TAB_MAX_GROUPS) void k_tabulate_finish(const GfTabPartial *__restrict__ partials, const uint32_t nPartials,
                                                                       GfTabSummary *__restrict__ summary, const int accumulate, const int64_t nCells)
{
    __shared__ GfTabPartial parts[GF_TAB_MAX_GROUPS / 64];
    const uint32_t tid = threadIdx.x;
    TabPartD d;
    gf_tab_part_start(d);
    if (tid < nPartials) d = tabFromPartial(partials[tid]);
    tabWaveMerge(d);
    if ((tid & 63) == 0) tabToPartial(d, parts[tid >> 6]);
    __syncthreads();
    if (tid != 0) return;
    for (uint32_t w = 1; w < GF_TAB_MAX_GROUPS / 64; w++) gf_tab_part_merge(d, tabFromPartial(parts[w]));
    GfTabSummary out = *summary;                                                   // (looked at only when accumulating)
    gf_tab_finish(out, d, accumulate, nCells);
    *summary = out;
}

template <typename T, bool LDS, bool UNIT>
hipError_t tabDenseLaunch(const GfTabDenseArgs &a, unsigned groups, size_t dyn, int64_t head, int64_t nVec, hipStream_t stream)
{
    static GfDynLdsOptIn optIn;                                                    // (one per instantiation)
    if (LDS) {
        const hipError_t e = gf_opt_in_dyn_lds(k_tabulate_dense<T, LDS, UNIT>, dyn, optIn);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_tabulate_dense<T, LDS, UNIT>), dim3(groups), dim3(GF_TAB_THREADS), dyn, stream, a.g, (const T *)a.block, a.counter, a.partials,
                       head, nVec);
    return hipGetLastError();
}

template <typename T>
hipError_t tabDense(const GfTabDenseArgs &a, hipStream_t stream)
{
    constexpr int64_t CPV = 16 / (int64_t)sizeof(T);
    const uintptr_t addr = (uintptr_t)a.block;
    int64_t head = (int64_t)(((16u - (addr & 15u)) & 15u) / sizeof(T));
    if (head > a.g.nCells) head = a.g.nCells;
    const int64_t nVec = (a.g.nCells - head) / CPV;
    const int64_t lanes = nVec > 8 ? nVec : 8;                                     // (head and tail: fewer than 8 cells each)
    int64_t groups = (lanes + GF_TAB_THREADS - 1) / GF_TAB_THREADS;
    if (groups > GF_TAB_MAX_GROUPS) groups = GF_TAB_MAX_GROUPS;
    const int64_t trips = (nVec + groups * GF_TAB_THREADS - 1) / (groups * GF_TAB_THREADS);
    if (trips * CPV >= ((int64_t)1 << 31)) return hipErrorInvalidValue;            // (a lane's own cell numbers are int32; GF_TAB_MAX_CELLS keeps far below)
    const uint32_t nBins = (uint32_t)a.g.nCounter + 1u;
    const bool lds = nBins <= GF_TAB_LDS_MAX_BINS;
    const size_t dyn = (lds ? (size_t)((nBins + 3u) & ~3u) * 4 : 0) + TAB_WAVES * sizeof(GfTabPartial);
    hipError_t e;
    if constexpr (std::is_floating_point_v<T>) {
        e = lds ? tabDenseLaunch<T, true, false>(a, (unsigned)groups, dyn, head, nVec, stream)
                : tabDenseLaunch<T, false, false>(a, (unsigned)groups, dyn, head, nVec, stream);
    } else {
        const bool unit = a.g.scaleUsed == 1.0;
        e = lds ? (unit ? tabDenseLaunch<T, true, true>(a, (unsigned)groups, dyn, head, nVec, stream)
                        : tabDenseLaunch<T, true, false>(a, (unsigned)groups, dyn, head, nVec, stream))
                : (unit ? tabDenseLaunch<T, false, true>(a, (unsigned)groups, dyn, head, nVec, stream)
                        : tabDenseLaunch<T, false, false>(a, (unsigned)groups, dyn, head, nVec, stream));
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tabulate_finish, dim3(1), dim3(GF_TAB_MAX_GROUPS), 0, stream, a.partials, (uint32_t)groups, a.summary, a.accumulate,
                       a.g.nCells);
    return hipGetLastError();
}

// ---------------------------------------------------------------- the symbol form: sort

constexpr uint32_t ST = GF_TAB_SORT_THREADS;

__device__ __forceinline__ size_t tabGroup() { return (size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x; }

// the exclusive prefix of x over the workgroup's ST lanes, and their total; waveTot: ST / 64 words of LDS
__device__ __forceinline__ uint32_t tabBlockExclScan(uint32_t x, uint32_t *waveTot, uint32_t &total)
{
    const uint32_t incl = gf_wave_incl_scan(x), w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) waveTot[w] = incl;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (uint32_t k = 0; k < ST / 64; k++) {
        const uint32_t t = waveTot[k];
        if (k < w) base += t;
        total += t;
    }
    __syncthreads();
    return base + incl - x;
}

__global__ __launch_bounds__(ST) void k_tab_keys_short(const int16_t *__restrict__ block, uint32_t *__restrict__ keys, const uint32_t n)
{
    const size_t i = tabGroup() * ST + threadIdx.x;
    if (i < n) keys[i] = gf_tab_symbol_i16(block[i]);
}

// workgroup w counts the digit `shift / 8` of keys [w * share, (w + 1) * share) into hist[digit * nWg + w]
__global__ __launch_bounds__(ST) void k_tab_digit_hist(const uint32_t *__restrict__ keys, const uint32_t n, const uint32_t share, const uint32_t shift,
                                                       uint32_t *__restrict__ hist, const uint32_t nWg)
{
    __shared__ uint32_t h[256];
    const size_t wg = tabGroup();
    if (wg >= nWg) return;                                                         // (the grid's padding; workgroup-uniform)
    const uint32_t tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const uint32_t begin = (uint32_t)wg * share, end = n - begin < share ? n : begin + share;
    for (uint32_t i = begin + tid; i < end; i += ST) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    __syncthreads();
    hist[(size_t)tid * nWg + wg] = h[tid];
}

// PHASE 0: sums[b] = the sum of data[b * GF_TAB_SCAN_BLOCK ..); PHASE 1 (one workgroup): sums -> their exclusive scan, *total (may
// be null) = everything; PHASE 2: data -> its exclusive scan, on sums[b]
template <int PHASE>
__global__ __launch_bounds__(ST) void k_tab_digit_scan(uint32_t *__restrict__ data, const size_t len, uint32_t *__restrict__ sums, const size_t nSums,
                                                       uint32_t *__restrict__ total)
{
    __shared__ uint32_t waveTot[ST / 64];
    const uint32_t tid = threadIdx.x;
    constexpr uint32_t PER = GF_TAB_SCAN_BLOCK / ST;
    if constexpr (PHASE == 1) {
        uint32_t carry = 0;
        for (size_t c = 0; c < nSums; c += ST) {
            const bool in = c + tid < nSums;
            const uint32_t x = in ? sums[c + tid] : 0u;
            uint32_t all;
            const uint32_t e = tabBlockExclScan(x, waveTot, all);
            if (in) sums[c + tid] = carry + e;
            carry += all;
        }
        if (tid == 0 && total) *total = carry;
    } else {
        const size_t b = tabGroup();
        if (b >= nSums) return;                                                    // (workgroup-uniform)
        const size_t i0 = b * GF_TAB_SCAN_BLOCK + (size_t)tid * PER;
        uint32_t x[PER], s = 0;
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) {
            x[k] = i0 + k < len ? data[i0 + k] : 0u;
            s += x[k];
        }
        uint32_t all;
        uint32_t e = tabBlockExclScan(s, waveTot, all);
        if constexpr (PHASE == 0) {
            if (tid == 0) sums[b] = all;
        } else {
            e += sums[b];
#pragma unroll
            for (uint32_t k = 0; k < PER; k++) {
                if (i0 + k < len) data[i0 + k] = e;
                e += x[k];
            }
        }
    }
}

// offs: the scanned hist.  A round: the ST keys behind one another; a key's place is its digit's running offset + the keys of the
// digit in the waves in front + those in front of it in its own wave (ballots): equal digits stay in input order
__global__ __launch_bounds__(ST) void k_tab_scatter(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, const uint32_t n, const uint32_t share,
                                                    const uint32_t shift, const uint32_t *__restrict__ offs, const uint32_t nWg)
{
    __shared__ uint32_t running[256];
    __shared__ uint32_t cnt[ST / 64][256];
    const size_t wg = tabGroup();
    if (wg >= nWg) return;                                                         // (workgroup-uniform)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    running[tid] = offs[(size_t)tid * nWg + wg];
#pragma unroll
    for (uint32_t k = 0; k < ST / 64; k++) cnt[k][tid] = 0;
    __syncthreads();
    const uint32_t begin = (uint32_t)wg * share, end = n - begin < share ? n : begin + share;
    for (uint32_t r0 = begin; r0 < end; r0 += ST) {
        const uint32_t i = r0 + tid;
        const bool valid = i < end;
        const uint32_t key = valid ? in[i] : 0u, d = (key >> shift) & 255u;
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0) cnt[w][d] = (uint32_t)__popcll(same);
        __syncthreads();
        {
            uint32_t acc = running[tid];
#pragma unroll
            for (uint32_t k = 0; k < ST / 64; k++) {
                const uint32_t t = cnt[k][tid];
                cnt[k][tid] = acc;
                acc += t;
            }
            running[tid] = acc;
        }
        __syncthreads();
        if (valid) {
            const uint32_t to = cnt[w][d] + rank;
            if (to < n) out[to] = key;                                             // (always: the offsets are the counts of these keys)
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < ST / 64; k++) cnt[k][tid] = 0;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- the symbol form: runs of the sorted keys

constexpr uint32_t RUN_PER = GF_TAB_RUN_BLOCK / ST;

// PHASE 0: heads[b] = run heads among keys [b * GF_TAB_RUN_BLOCK ..); PHASE 1 (heads scanned): head j of the whole at key i:
// starts[j] = i, symbols[j] = the key while j < cap
template <int PHASE>
__global__ __launch_bounds__(ST) void k_tab_runs(const uint32_t *__restrict__ keys, const uint32_t n, uint32_t *__restrict__ heads,
                                                 uint32_t *__restrict__ starts, uint32_t *__restrict__ symbols, const uint64_t cap, const size_t nBlocks)
{
    __shared__ uint32_t waveTot[ST / 64];
    const size_t b = tabGroup();
    if (b >= nBlocks) return;                                                      // (workgroup-uniform)
    const uint32_t tid = threadIdx.x;
    const uint64_t i0 = (uint64_t)b * GF_TAB_RUN_BLOCK + (uint64_t)tid * RUN_PER;
    uint32_t key[RUN_PER], isHead = 0, nHeads = 0;
    uint32_t prev = (i0 > 0 && i0 <= n) ? keys[i0 - 1] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < RUN_PER; k++) {
        const uint64_t i = i0 + k;
        key[k] = i < n ? keys[i] : 0u;
        const bool hd = i < n && (i == 0 || key[k] != prev);
        isHead |= (uint32_t)hd << k;
        nHeads += hd;
        prev = key[k];
    }
    uint32_t all;
    uint32_t j = tabBlockExclScan(nHeads, waveTot, all);
    if constexpr (PHASE == 0) {
        if (tid == 0) heads[b] = all;
    } else {
        j += heads[b];
#pragma unroll
        for (uint32_t k = 0; k < RUN_PER; k++)
            if ((isHead >> k) & 1u) {
                starts[j] = (uint32_t)(i0 + k);
                if (j < cap) symbols[j] = key[k];
                j++;
            }
    }
}

// one lane, behind the scan of the heads: the scalars that are known now, zeroes for phase 2's atomics, and the end of the last run
__global__ void k_tab_runs_head(const uint32_t *__restrict__ nSym, const uint32_t n, const uint64_t cap, uint32_t *__restrict__ starts,
                                GfTabSymbols *__restrict__ summary)
{
    const uint32_t total = *nSym;
    starts[total] = n;
    summary->nSamples = n, summary->nSymbols = total, summary->nUnique = 0, summary->nRepeated = 0;
    summary->nWritten = total < cap ? total : (int64_t)cap;
    summary->maxCount = 0, summary->reserved = 0;
}

// symbol j's count = starts[j + 1] - starts[j]; the scalars by integer atomics (any order gives the same)
__global__ __launch_bounds__(ST) void k_tab_run_counts(const uint32_t *__restrict__ nSym, const uint32_t *__restrict__ starts, int32_t *__restrict__ counts,
                                                       const uint64_t cap, GfTabSymbols *__restrict__ summary)
{
    const uint32_t total = *nSym;
    uint32_t unique = 0, repeated = 0, most = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * ST + threadIdx.x; j < total; j += (uint64_t)gridDim.x * ST) {
        const uint32_t c = starts[j + 1] - starts[j];
        if (j < cap) counts[j] = (int32_t)c;
        unique += c == 1u, repeated += c != 1u;
        most = c > most ? c : most;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unique += __shfl_down(unique, off, 64), repeated += __shfl_down(repeated, off, 64);
        const uint32_t m = __shfl_down(most, off, 64);
        most = m > most ? m : most;
    }
    if ((threadIdx.x & 63) == 0) {
        if (unique) atomicAdd((unsigned long long *)&summary->nUnique, (unsigned long long)unique);
        if (repeated) atomicAdd((unsigned long long *)&summary->nRepeated, (unsigned long long)repeated);
        if (most) atomicMax(&summary->maxCount, (int32_t)most);
    }
}

#define TAB_LAUNCHED()                          \
    do {                                        \
        const hipError_t e_ = hipGetLastError(); \
        if (e_ != hipSuccess) return e_;        \
    } while (0)

// data[0 .. len) -> its exclusive scan; sums: room for ceil(len / GF_TAB_SCAN_BLOCK) words
hipError_t tabScan(uint32_t *data, size_t len, uint32_t *sums, uint32_t *total, hipStream_t stream)
{
    const size_t nSums = (len + GF_TAB_SCAN_BLOCK - 1) / GF_TAB_SCAN_BLOCK;
    hipLaunchKernelGGL(k_tab_digit_scan<0>, gf_tile_grid(nSums), dim3(ST), 0, stream, data, len, sums, nSums, (uint32_t *)nullptr);
    TAB_LAUNCHED();
    hipLaunchKernelGGL(k_tab_digit_scan<1>, dim3(1), dim3(ST), 0, stream, data, len, sums, nSums, total);
    TAB_LAUNCHED();
    hipLaunchKernelGGL(k_tab_digit_scan<2>, gf_tile_grid(nSums), dim3(ST), 0, stream, data, len, sums, nSums, (uint32_t *)nullptr);
    return hipGetLastError();
}

// ---------------------------------------------------------------- the symbol form: two tables merged

constexpr uint32_t MERGE_PER = GF_TAB_MERGE_BLOCK / ST;
constexpr uint32_t MERGE_WIN = GF_TAB_MERGE_BLOCK + 4;                            // gf_tab_merge_window's bound

struct TabMergeIn {
    const uint32_t *symA, *symB;
    const int32_t *cntA, *cntB;
    const GfTabSymbols *sumA, *sumB;
    uint32_t capA, capB, noSamplesIsEmpty;
};
__device__ __forceinline__ uint32_t tabLenA(const TabMergeIn &in) { return gf_tab_table_len(in.sumA, in.capA, in.noSamplesIsEmpty & 1u); }
__device__ __forceinline__ uint32_t tabLenB(const TabMergeIn &in) { return gf_tab_table_len(in.sumB, in.capB, in.noSamplesIsEmpty & 2u); }

// splits[i] = the split of the merged sequence at position min(i * GF_TAB_MERGE_BLOCK, nA + nB), i = 0 .. nChunks: one lane each,
// so that the searches through the tables, a chain of dependent loads each, all run at once and no workgroup of k_tab_merge waits
// for its own
__global__ __launch_bounds__(ST) void k_tab_merge_splits(const TabMergeIn in, uint32_t *__restrict__ splits, const size_t nChunks)
{
    const size_t i = tabGroup() * ST + threadIdx.x;
    if (i > nChunks) return;
    const uint32_t nA = tabLenA(in), nB = tabLenB(in);
    const uint64_t n = (uint64_t)nA + nB, d = (uint64_t)i * GF_TAB_MERGE_BLOCK;
    splits[i] = gf_tab_merge_split(in.symA, nA, in.symB, nB, d < n ? d : n);
}

// Workgroup b owns positions [b * GF_TAB_MERGE_BLOCK ..) of the merged sequence (gvrs_tabulate_common.h); the grid is laid out for
// capA + capB positions and the workgroups behind the tables' real lengths, which only the device knows, have nothing to do.  With
// the chunk's two splits from k_tab_merge_splits the workgroup brings the chunk's window into LDS, and every lane finds the
// split of its own MERGE_PER positions there and walks them by the pair rule.  PHASE 0: heads[b] = the chunk's heads (scanned by
// k_tab_digit_scan); PHASE 1: head j of the whole goes to symbols[j] / counts[j] while j < cap, and the scalars over the counts
// > 0 are added to the summary by integer atomics (k_tab_merge_head has written the rest of it).
template <int PHASE>
__global__ __launch_bounds__(ST) void k_tab_merge(const TabMergeIn in, const uint32_t *__restrict__ splits, uint32_t *__restrict__ heads,
                                                  uint32_t *__restrict__ symbols, int32_t *__restrict__ counts, const uint64_t cap,
                                                  GfTabSymbols *__restrict__ summary, const size_t nChunks)
{
    __shared__ uint32_t sym[MERGE_WIN];
    __shared__ int32_t cnt[MERGE_WIN];
    __shared__ uint32_t waveTot[ST / 64];
    const size_t b = tabGroup();
    if (b >= nChunks) return;                                                      // (the grid's padding; workgroup-uniform)
    const uint32_t tid = threadIdx.x;
    const uint32_t nA = tabLenA(in), nB = tabLenB(in);
    const uint64_t n = (uint64_t)nA + nB, d0 = (uint64_t)b * GF_TAB_MERGE_BLOCK;
    if (d0 >= n) {                                                                 // (workgroup-uniform)
        if (PHASE == 0 && tid == 0) heads[b] = 0;
        return;
    }
    const uint64_t d1 = n - d0 < GF_TAB_MERGE_BLOCK ? n : d0 + GF_TAB_MERGE_BLOCK;
    const GfTabMergeWindow w = gf_tab_merge_window(nA, nB, d0, splits[b], d1, splits[b + 1]);
    const uint32_t lA = w.a1 - w.a0, lB = w.b1 - w.b0;                             // lA + lB <= MERGE_WIN
    for (uint32_t i = tid; i < lA + lB; i += ST) {
        const bool isA = i < lA;
        sym[i] = isA ? in.symA[w.a0 + i] : in.symB[w.b0 + (i - lA)];
        cnt[i] = isA ? in.cntA[w.a0 + i] : in.cntB[w.b0 + (i - lA)];
    }
    __syncthreads();
    const uint32_t len = (uint32_t)(d1 - d0), at = tid * MERGE_PER;                // the lane's positions: [at, at + steps) of the chunk
    const uint32_t steps = at >= len ? 0u : len - at < MERGE_PER ? len - at : MERGE_PER;
    uint32_t ia = 0, ib = 0;
    if (steps) {
        ia = gf_tab_merge_split(sym, lA, sym + lA, lB, (uint64_t)w.pre + at);
        ib = w.pre + at - ia;
    }
    uint32_t hs[MERGE_PER];
    int32_t hc[MERGE_PER];
    const uint32_t nHeads = gf_tab_merge_run(sym, cnt, lA, sym + lA, cnt + lA, lB, ia, ib, steps, [&](uint32_t k, uint32_t s, int32_t c) {
#pragma unroll
        for (uint32_t q = 0; q < MERGE_PER; q++)
            if (q == k) hs[q] = s, hc[q] = c;
    });
    uint32_t all;
    uint64_t j = tabBlockExclScan(nHeads, waveTot, all);
    if constexpr (PHASE == 0) {
        if (tid == 0) heads[b] = all;
    } else {
        j += heads[b];
        uint32_t unique = 0, repeated = 0;
        int32_t most = 0;
#pragma unroll
        for (uint32_t q = 0; q < MERGE_PER; q++)
            if (q < nHeads) {
                if (j < cap) symbols[j] = hs[q], counts[j] = hc[q];
                gf_tab_count_scalars(hc[q], unique, repeated, most);
                j++;
            }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            unique += __shfl_down(unique, off, 64), repeated += __shfl_down(repeated, off, 64);
            const int32_t m = __shfl_down(most, off, 64);
            most = m > most ? m : most;
        }
        if ((tid & 63) == 0) {
            if (unique) atomicAdd((unsigned long long *)&summary->nUnique, (unsigned long long)unique);
            if (repeated) atomicAdd((unsigned long long *)&summary->nRepeated, (unsigned long long)repeated);
            if (most) atomicMax(&summary->maxCount, most);
        }
    }
}

// one lane, behind the scan of the heads: the summary but for the scalars that phase 1 adds up
__global__ void k_tab_merge_head(const TabMergeIn in, const uint32_t *__restrict__ nSym, const uint64_t cap, GfTabSymbols *__restrict__ summary)
{
    // (a table that is empty for want of samples gives nothing, its flag included)
    const GfTabSymbols *a = (in.noSamplesIsEmpty & 1u) && in.sumA && in.sumA->nSamples == 0 ? nullptr : in.sumA;
    const GfTabSymbols *b = (in.noSamplesIsEmpty & 2u) && in.sumB && in.sumB->nSamples == 0 ? nullptr : in.sumB;
    GfTabSymbols out;
    gf_tab_merge_summary(out, a, tabLenA(in), b, tabLenB(in), *nSym, cap);
    *summary = out;
}

// ---------------------------------------------------------------- the symbol form: a SHORT block by counters

// k_tabulate_dense's scheme on the 65,536 values a SHORT cell can take: persistent workgroups, 16-byte loads of 8 cells, the cells in
// front of the first 16-byte boundary and behind the last whole load one a lane (the block need only be 2-byte aligned).  The
// counters of the window GF_TAB_SHORT_WIN_LO .. _HI are private to the workgroup in LDS and the non-zero ones are flushed once; a
// cell outside the window is one global atomic.  counter: 65,536 words, zeroed by the launcher, indexed by gf_tab_short_slot.
__global__ __launch_bounds__(GF_TAB_THREADS) void k_tab_short_counts(const int16_t *__restrict__ block, int32_t *__restrict__ counter, const int64_t nCells,
                                                                     const int64_t head, const int64_t nVec)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t tabWin[];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < (uint32_t)GF_TAB_SHORT_WIN; i += GF_TAB_THREADS) tabWin[i] = 0;
    __syncthreads();
    auto count = [&](int16_t v) {
        const uint32_t ws = gf_tab_short_win_slot(v);
        if (ws < (uint32_t)GF_TAB_SHORT_WIN) atomicAdd(&tabWin[ws], 1u);
        else atomicAdd(&counter[gf_tab_short_slot(v)], 1);
    };
    const int64_t gid = (int64_t)blockIdx.x * GF_TAB_THREADS + tid, stride = (int64_t)gridDim.x * GF_TAB_THREADS;
    if (gid < head) count(block[gid]);
    const uint4 *vec = reinterpret_cast<const uint4 *>(block + head);
    for (int64_t v = gid; v < nVec; v += stride) {
        const uint4 x = vec[v];
#pragma unroll
        for (int c = 0; c < 8; c++) count(tabCellOf<int16_t>(x, c));
    }
    const int64_t tail0 = head + nVec * 8;
    if (gid < nCells - tail0) count(block[tail0 + gid]);
    __syncthreads();
    for (uint32_t i = tid; i < (uint32_t)GF_TAB_SHORT_WIN; i += GF_TAB_THREADS) {
        const uint32_t c = tabWin[i];
        if (c) atomicAdd(&counter[gf_tab_short_slot(gf_tab_short_of_win_slot(i))], (int32_t)c);
    }
}

// one workgroup: the table of the 65,536 counters -- slot s is the symbol of (int16) s sign-extended, the slots' order is the symbols'
// ascending unsigned order, counters equal to 0 are left out -- and its summary, whole.  A lane owns 64 slots behind one another.
__global__ __launch_bounds__(GF_TAB_COMPACT_THREADS) void k_tab_short_compact(const int32_t *__restrict__ counter, const int64_t nSamples,
                                                                              uint32_t *__restrict__ symbols, int32_t *__restrict__ counts, const uint64_t cap,
                                                                              GfTabSymbols *__restrict__ summary)
{
    constexpr uint32_t WAVES = GF_TAB_COMPACT_THREADS / 64, PER = 65536 / GF_TAB_COMPACT_THREADS;
    __shared__ uint32_t waveTot[WAVES], waveUnique[WAVES], waveRepeated[WAVES];
    __shared__ int32_t waveMost[WAVES];
    const uint32_t tid = threadIdx.x, s0 = tid * PER;
    uint32_t mine = 0, unique = 0, repeated = 0;
    int32_t most = 0;
    for (uint32_t k = 0; k < PER; k++) {
        const int32_t c = counter[s0 + k];
        mine += c != 0;
        gf_tab_count_scalars(c, unique, repeated, most);
    }
    const uint32_t incl = gf_wave_incl_scan(mine);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unique += __shfl_down(unique, off, 64), repeated += __shfl_down(repeated, off, 64);
        const int32_t m = __shfl_down(most, off, 64);
        most = m > most ? m : most;
    }
    if ((tid & 63) == 63) waveTot[tid >> 6] = incl;
    if ((tid & 63) == 0) waveUnique[tid >> 6] = unique, waveRepeated[tid >> 6] = repeated, waveMost[tid >> 6] = most;
    __syncthreads();
    uint64_t j = incl - mine;
    uint32_t total = 0;
    for (uint32_t w = 0; w < WAVES; w++) {
        if (w < (tid >> 6)) j += waveTot[w];
        total += waveTot[w];
    }
    for (uint32_t k = 0; k < PER; k++) {
        const int32_t c = counter[s0 + k];
        if (c == 0) continue;
        if (j < cap) symbols[j] = gf_tab_symbol_i16((int16_t)(uint16_t)(s0 + k)), counts[j] = c;
        j++;
    }
    if (tid != 0) return;
    GfTabSymbols out;
    out.nSamples = nSamples, out.nSymbols = total, out.nUnique = 0, out.nRepeated = 0, out.maxCount = 0, out.reserved = 0;
    out.nWritten = total < cap ? total : (int64_t)cap;
    for (uint32_t w = 0; w < WAVES; w++) {
        out.nUnique += waveUnique[w], out.nRepeated += waveRepeated[w];
        out.maxCount = waveMost[w] > out.maxCount ? waveMost[w] : out.maxCount;
    }
    *summary = out;
}

}  // namespace

hipError_t gf_launch_tabulate_dense(const GfTabDenseArgs &a, hipStream_t stream)
{
    if (!a.counter || !a.partials || !a.summary || a.g.nCells < 0 || a.g.nCounter < 0 || (a.g.nCells > 0 && !a.block)) return hipErrorInvalidValue;
    switch (a.g.elemType) {
    case 0: return tabDense<int32_t>(a, stream);
    case 1: return tabDense<int16_t>(a, stream);
    case 2: return tabDense<float>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

GfTabSortPlan gf_tab_sort_plan(uint32_t n)
{
    GfTabSortPlan p{};
    p.share = gf_tab_sort_share(n);
    p.nWg = (n + p.share - 1u) / p.share;
    p.histWords = (size_t)256 * p.nWg;
    p.nRunBlocks = ((size_t)n + GF_TAB_RUN_BLOCK - 1) / GF_TAB_RUN_BLOCK;
    const size_t a = (p.histWords + GF_TAB_SCAN_BLOCK - 1) / GF_TAB_SCAN_BLOCK, b = (p.nRunBlocks + GF_TAB_SCAN_BLOCK - 1) / GF_TAB_SCAN_BLOCK;
    p.sumWords = a > b ? a : b;
    return p;
}

hipError_t gf_launch_tab_symbols(const GfTabSymbolsArgs &a, hipStream_t stream)
{
    if (!a.block || a.n < 1 || a.n > 0x7fffffffu || !a.keysA || !a.keysB || !a.hist || !a.sums || !a.heads || !a.nSym || !a.summary ||
        (a.cap && (!a.symbols || !a.counts)))
        return hipErrorInvalidValue;
    const GfTabSortPlan p = gf_tab_sort_plan(a.n);
    const uint32_t *cur;
    switch (a.elemType) {
    case 0: case 2: cur = (const uint32_t *)a.block; break;                        // INT: the cells; FLOAT: their raw bits
    case 1:
        hipLaunchKernelGGL(k_tab_keys_short, gf_tile_grid(((size_t)a.n + ST - 1) / ST), dim3(ST), 0, stream, (const int16_t *)a.block, a.keysB, a.n);
        TAB_LAUNCHED();
        cur = a.keysB;
        break;
    default: return hipErrorInvalidValue;
    }
    // four passes: cur -> A -> B -> A -> B; the block itself is only ever read
    for (uint32_t pass = 0; pass < 4; pass++) {
        uint32_t *to = (pass & 1u) ? a.keysB : a.keysA;
        hipLaunchKernelGGL(k_tab_digit_hist, gf_tile_grid(p.nWg), dim3(ST), 0, stream, cur, a.n, p.share, 8u * pass, a.hist, p.nWg);
        TAB_LAUNCHED();
        const hipError_t e = tabScan(a.hist, p.histWords, a.sums, nullptr, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_tab_scatter, gf_tile_grid(p.nWg), dim3(ST), 0, stream, cur, to, a.n, p.share, 8u * pass, a.hist, p.nWg);
        TAB_LAUNCHED();
        cur = to;
    }
    // sorted in B; A (n + 1 words) takes the runs' starts
    hipLaunchKernelGGL(k_tab_runs<0>, gf_tile_grid(p.nRunBlocks), dim3(ST), 0, stream, a.keysB, a.n, a.heads, a.keysA, a.symbols, (uint64_t)a.cap,
                       p.nRunBlocks);
    TAB_LAUNCHED();
    const hipError_t e = tabScan(a.heads, p.nRunBlocks, a.sums, a.nSym, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tab_runs_head, dim3(1), dim3(1), 0, stream, a.nSym, a.n, (uint64_t)a.cap, a.keysA, a.summary);
    TAB_LAUNCHED();
    hipLaunchKernelGGL(k_tab_runs<1>, gf_tile_grid(p.nRunBlocks), dim3(ST), 0, stream, a.keysB, a.n, a.heads, a.keysA, a.symbols, (uint64_t)a.cap,
                       p.nRunBlocks);
    TAB_LAUNCHED();
    const size_t groups = ((size_t)a.n + ST - 1) / ST;
    hipLaunchKernelGGL(k_tab_run_counts, dim3((unsigned)(groups < 2048 ? groups : 2048)), dim3(ST), 0, stream, a.nSym, a.keysA, a.counts, (uint64_t)a.cap,
                       a.summary);
    return hipGetLastError();
}

size_t gf_tab_merge_chunks(uint32_t capA, uint32_t capB)
{
    const size_t n = ((size_t)capA + capB + GF_TAB_MERGE_BLOCK - 1) / GF_TAB_MERGE_BLOCK;
    return n ? n : 1;
}

hipError_t gf_launch_tab_merge(const GfTabMergeArgs &a, hipStream_t stream)
{
    if (!a.splits || !a.heads || !a.sums || !a.nSym || !a.summary || (a.cap && (!a.symbols || !a.counts)) || a.capA > 0x7fffffffu || a.capB > 0x7fffffffu ||
        (a.capA && (!a.symA || !a.cntA)) || (a.capB && (!a.symB || !a.cntB)))
        return hipErrorInvalidValue;
    TabMergeIn in{};
    in.symA = a.symA, in.cntA = a.cntA, in.sumA = a.sumA, in.capA = a.sumA ? a.capA : 0u;
    in.symB = a.symB, in.cntB = a.cntB, in.sumB = a.sumB, in.capB = a.sumB ? a.capB : 0u;
    in.noSamplesIsEmpty = a.noSamplesIsEmpty;
    const size_t nChunks = gf_tab_merge_chunks(in.capA, in.capB);
    hipLaunchKernelGGL(k_tab_merge_splits, gf_tile_grid((nChunks + 1 + ST - 1) / ST), dim3(ST), 0, stream, in, a.splits, nChunks);
    TAB_LAUNCHED();
    hipLaunchKernelGGL(k_tab_merge<0>, gf_tile_grid(nChunks), dim3(ST), 0, stream, in, a.splits, a.heads, a.symbols, a.counts, (uint64_t)a.cap,
                       a.summary, nChunks);
    TAB_LAUNCHED();
    const hipError_t e = tabScan(a.heads, nChunks, a.sums, a.nSym, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tab_merge_head, dim3(1), dim3(1), 0, stream, in, a.nSym, (uint64_t)a.cap, a.summary);
    TAB_LAUNCHED();
    hipLaunchKernelGGL(k_tab_merge<1>, gf_tile_grid(nChunks), dim3(ST), 0, stream, in, a.splits, a.heads, a.symbols, a.counts, (uint64_t)a.cap,
                       a.summary, nChunks);
    return hipGetLastError();
}

hipError_t gf_launch_tab_short(const GfTabShortArgs &a, hipStream_t stream)
{
    if (!a.block || a.n < 1 || a.n > 0x7fffffffu || ((uintptr_t)a.block & 1) != 0 || !a.counter || !a.summary || (a.cap && (!a.symbols || !a.counts)))
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.counter, 0, 65536 * sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    const int64_t nCells = a.n;
    int64_t head = (int64_t)(((16u - ((uintptr_t)a.block & 15u)) & 15u) / 2u);
    if (head > nCells) head = nCells;
    const int64_t nVec = (nCells - head) / 8;
    const int64_t lanes = nVec > 8 ? nVec : 8;                                     // (head and tail: fewer than 8 cells each)
    int64_t groups = (lanes + GF_TAB_THREADS - 1) / GF_TAB_THREADS;
    if (groups > GF_TAB_SHORT_MAX_GROUPS) groups = GF_TAB_SHORT_MAX_GROUPS;
    constexpr size_t dyn = (size_t)GF_TAB_SHORT_WIN * 4;
    static GfDynLdsOptIn optIn;
    if ((e = gf_opt_in_dyn_lds(k_tab_short_counts, dyn, optIn)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_tab_short_counts, dim3((unsigned)groups), dim3(GF_TAB_THREADS), dyn, stream, (const int16_t *)a.block, a.counter, nCells, head, nVec);
    TAB_LAUNCHED();
    hipLaunchKernelGGL(k_tab_short_compact, dim3(1), dim3(GF_TAB_COMPACT_THREADS), 0, stream, a.counter, nCells, a.symbols, a.counts, (uint64_t)a.cap,
                       a.summary);
    return hipGetLastError();
}
