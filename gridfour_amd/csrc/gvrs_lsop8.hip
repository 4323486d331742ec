// gvrs_lsop8.hip -- the LSOP08 codec (optimal 8-coefficient linear predictor over the 3 x 3 neighbourhood) for a batch of tiles on
// gfx950.
//
// Reference (core/src/main/java/org/gridfour/):
//   lsop/LsOptimalPredictor08.java:56-160    encode: initialiser stream, coefficients, interior stream
//   lsop/LsOptimalPredictor08.java:181-246   computeCoefficients: 9 x 9 normal equations with a Lagrange row
//   util/jama/LUDecomposition.java:70-134, 253-284   Crout LU with partial pivoting, solve
//   lsop/LsEncoder08.java:66-137, lsop/LsHeader.java:210-265   container: header + the two CodecM32 streams, as two legacy Huffman
//       segments back to back in one bit store (compression type 0) or as two zlib streams (type 1, the host's work)
//   lsop/LsDecoder08.java:71-163             decode
//
// Three kernels:
//   k_lsop8_predict      a tile per workgroup: tile -> seed, 8 float coefficients, residual ints [initialisers | interior]
//   k_lsop8_pack         a tile per workgroup: header + HuffmanEncoder(M32 of the initialisers) + HuffmanEncoder(M32 of the interior)
//   k_lsop8_reconstruct  a tile per wave: residual ints -> tile; prefix sums for rows 0, 1 and columns 0, 1, then the interior as a
//                        slope-1 wavefront: cell (r, c) needs (r, c-1) and (r-1, c) -- the predictor has no neighbour to the upper
//                        right --, so the rows of a band advance one column apart
// The containers are unpacked by k_lsop_unpack_m32 (gvrs_decode.hip) and k_lsop_streams / k_inflate (gvrs_inflate.hip), which take
// the coefficient count and the stream lengths from a GfLsopForm.
//
// Floating point: the normal equations are accumulated in FP64.  When max|v|^2 * cells < 2^53 every partial sum is an exact
// integer, so any order (and FMA) gives the reference's bits: a thread sums its share of the cells into 27 registers.  Otherwise
// 54 threads own one accumulator each and add in the reference's scan order with separately rounded multiply and add.  LU, solve and
// the float32 prediction follow the reference's operation order exactly (the library is built with -ffp-contract=off).  The estimate
// is (int)(p + 0.5f): a float32 addition and Java's cast (toward zero, NaN -> 0, saturating) -- not LSOP12's StrictMath.round.

#include <hip/hip_runtime.h>

#include "gvrs_kernels.h"
#include "huff_build.h"

namespace {

#include "gvrs_lsop_lu.h"

constexpr int L8_NZ = 10;                       // z0 .. z8 and z9 = 1
constexpr int L8_ACC = 54;                      // pairs (i, j), i <= j, without (9, 9)
constexpr int L8_THREADS = 256;

// (int) of a float as Java casts it: v_cvt_i32_f32 truncates toward zero, saturates and turns NaN into 0
__device__ __forceinline__ int32_t lsop8_estimate(float p)
{
    const float q = p + 0.5f;
    int32_t r;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(q));
    return r;
}

// z_i of the cell at idx as an offset into the tile (LsOptimalPredictor08.java:192-200)
__host__ __device__ constexpr int32_t lsop8_z_offset(int i, int32_t nC)
{
    return i == 0 ? 0 : i == 1 ? -1 : i == 2 ? -nC - 1 : i == 3 ? -nC : i == 4 ? -2 : i == 5 ? -nC - 2 : i == 6 ? -2 * nC - 2 : i == 7 ? -2 * nC - 1 : -2 * nC;
}

__device__ __forceinline__ uint32_t lsop8_n_init(uint32_t nR, uint32_t nC) { return 2u * nC + 2u * nR - 5u; }
__device__ __forceinline__ uint32_t lsop8_n_interior(uint32_t nR, uint32_t nC) { return (nR - 2u) * (nC - 2u); }

// initialiser element k -> its cell and the cell it is a difference against (:77-104)
__device__ __forceinline__ uint32_t lsop8_init_cell(uint32_t k, uint32_t nC, uint32_t *against)
{
    if (k < nC - 1u) { *against = k; return k + 1u; }                          // row 0: left differences
    k -= nC - 1u;
    if (k < nC) { *against = k == 0u ? 0u : nC + k - 1u; return nC + k; }         // row 1: the first against v[0]
    k -= nC;
    const uint32_t cell = (2u + (k >> 1)) * nC + (k & 1u);                      // rows 2 ..: column 0 against the cell above, column 1 against column 0
    *against = (k & 1u) ? cell - 1u : cell - nC;
    return cell;
}

struct PairTab8 {
    int8_t i[L8_ACC], j[L8_ACC];
};
constexpr PairTab8 make_pairs8()
{
    PairTab8 t{};
    int p = 0;
    for (int i = 0; i < L8_NZ - 1; i++)
        for (int j = i; j < L8_NZ; j++) { t.i[p] = (int8_t)i; t.j[p] = (int8_t)j; p++; }
    return t;
}
__device__ constexpr PairTab8 PAIRS8 = make_pairs8();

constexpr int L8_HALF = L8_ACC / 2;              // accumulators of a pair of waves (exact sums)

struct Lsop8Shared {
    double G[L8_ACC];
    double part[L8_THREADS / 64][L8_HALF];
    float u[8];
    uint32_t maxAbs;
    int32_t status;
};

struct GfLsop8PredictArgs {
    const int32_t *values;
    int32_t *residuals;        // per tile resStride ints: [initialisers | interior]
    size_t resStride;
    uint32_t *coefs;           // per tile 16 words: seed, 8 float bit patterns, 7 words of 0
    int32_t *status;
    size_t nTiles;
    int nRows, nCols;
};

// exact sums: waves 0 and 1 take accumulators 0 .. 26 (H = 0), waves 2 and 3 the other 27, each pair over all interior cells -- a
// thread every 128th cell, its 27 sums in registers (all 54 in one thread cost 171 VGPRs: two workgroups per CU)
template <int H>
__device__ __forceinline__ void lsop8_gram_half(const int32_t *__restrict__ v, uint32_t nC, uint32_t nInt, uint32_t idx, double (&acc)[L8_HALF])
{
    constexpr uint32_t STEP = L8_THREADS / 2;
    const uint32_t wI = nC - 2u;
    uint32_t r = idx / wI, c = idx - r * wI;
    const uint32_t dr = STEP / wI, dc = STEP - dr * wI;
    for (uint32_t e = idx; e < nInt; e += STEP) {
        const int32_t *at = v + (size_t)(r + 2u) * nC + c + 2u;
        double z[L8_NZ - 1];
#pragma unroll
        for (int i = 0; i < L8_NZ - 1; i++) z[i] = (double)at[lsop8_z_offset(i, (int32_t)nC)];
        int p = 0;
#pragma unroll
        for (int i = 0; i < L8_NZ - 1; i++) {
#pragma unroll
            for (int j = i; j < L8_NZ - 1; j++) {
                if (p / L8_HALF == H) acc[p % L8_HALF] = fma(z[i], z[j], acc[p % L8_HALF]);
                p++;
            }
            if (p / L8_HALF == H) acc[p % L8_HALF] += z[i];
            p++;
        }
        r += dr;
        c += dc;
        if (c >= wI) { c -= wI; r++; }
    }
}

// ------------------------------------------------------------------------------------------------
// k_lsop8_predict
// ------------------------------------------------------------------------------------------------
constexpr int L8_PREDICT_WAVES = 4;               // waves per SIMD the register budget is cut for: four workgroups per CU
__global__ __launch_bounds__(L8_THREADS, L8_PREDICT_WAVES) void k_lsop8_predict(GfLsop8PredictArgs a)
{
    __shared__ Lsop8Shared S;
    const int tid = threadIdx.x, lane = tid & 63, wave = (int)gf_wave_id();
    const uint32_t nR = (uint32_t)a.nRows, nC = (uint32_t)a.nCols, nCells = nR * nC;
    const uint32_t nInit = lsop8_n_init(nR, nC), nInt = lsop8_n_interior(nR, nC), wI = nC - 2u;

    for (size_t t = blockIdx.x; t < a.nTiles; t += gridDim.x) {
        const int32_t *__restrict__ v = a.values + t * (size_t)nCells;
        int32_t *__restrict__ res = a.residuals + t * a.resStride;
        __syncthreads();                                       // (the tile before is done with S)
        if (tid == 0) { S.maxAbs = 0; S.status = GF_K_OK; }
        __syncthreads();

        // initialiser stream and max |v|
        for (uint32_t k = tid; k < nInit; k += L8_THREADS) {
            uint32_t against;
            const uint32_t idx = lsop8_init_cell(k, nC, &against);
            res[k] = (int32_t)((uint32_t)v[idx] - (uint32_t)v[against]);
        }
        uint32_t m = 0;
        {
            // (sixteen bytes a load, four loads in flight: this is the tile's first trip from HBM)
            auto mag = [](uint32_t x) -> uint32_t { return (int32_t)x < 0 ? 0u - x : x; };
            const uint32_t n4 = nCells >> 2;
            const GfU4 *v4 = reinterpret_cast<const GfU4 *>(v);
#pragma unroll 4
            for (uint32_t i = tid; i < n4; i += L8_THREADS) {
                const GfU4 q = v4[i];
                m = max(max(m, mag(q.x)), max(mag(q.y), max(mag(q.z), mag(q.w))));
            }
            for (uint32_t i = (n4 << 2) + tid; i < nCells; i += L8_THREADS) m = max(m, mag((uint32_t)v[i]));
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = max(m, gf_lane_xor(m, o));
        if (lane == 0) atomicMax(&S.maxAbs, m);
        __syncthreads();

        // normal equations (:186-210)
        const double bound = (double)S.maxAbs * (double)S.maxAbs * (double)nInt;
        if (bound < 9007199254740992.0) {
            double acc[L8_HALF];
#pragma unroll
            for (int p = 0; p < L8_HALF; p++) acc[p] = 0.0;
            if (wave < 2) lsop8_gram_half<0>(v, nC, nInt, (uint32_t)tid, acc);
            else lsop8_gram_half<1>(v, nC, nInt, (uint32_t)tid - L8_THREADS / 2, acc);
#pragma unroll
            for (int p = 0; p < L8_HALF; p++) {
                double x = acc[p];
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
                if (lane == 0) S.part[wave][p] = x;
            }
            __syncthreads();
            if (tid < L8_ACC) {
                const int h = tid / L8_HALF, p = tid % L8_HALF;
                S.G[tid] = S.part[2 * h][p] + S.part[2 * h + 1][p];
            }
        } else if (tid < L8_ACC) {
            // inexact sums: one accumulator per thread, the reference's scan order, multiply and add rounded separately
            const int pi = PAIRS8.i[tid], pj = PAIRS8.j[tid];
            const int32_t oi = lsop8_z_offset(pi, (int32_t)nC), oj = pj == L8_NZ - 1 ? 0 : lsop8_z_offset(pj, (int32_t)nC);
            double acc = 0.0;
            for (uint32_t r = 2; r < nR; r++) {
                const int32_t *row = v + (size_t)r * nC;
                for (uint32_t c = 2; c < nC; c++) {
                    const double zi = (double)row[(int32_t)c + oi];
                    const double zj = pj == L8_NZ - 1 ? 1.0 : (double)row[(int32_t)c + oj];
                    acc = __dadd_rn(acc, pj == L8_NZ - 1 ? zi : __dmul_rn(zi, zj));
                }
            }
            S.G[tid] = acc;
        }
        __syncthreads();

        // 9 x 9 bordered system, LU, solve (:211-245) by wave 0
        if (wave == 0) lsop_lu_solve_wave<L8_NZ - 1>(S, lane);
        __syncthreads();
        if (S.status != GF_K_OK) {
            if (tid == 0) a.status[t] = S.status;
            continue;
        }
        float u[8];
#pragma unroll
        for (int i = 0; i < 8; i++) u[i] = S.u[i];
        if (tid < 16) a.coefs[t * 16 + tid] = tid == 0 ? (uint32_t)v[0] : tid <= 8 ? __float_as_uint(S.u[tid - 1]) : 0u;

        // interior stream (:135-150): every cell on its own; four cells per thread in flight (their 36 loads are independent)
        {
            constexpr int U = 4;
            uint32_t r = (uint32_t)tid / wI, c = (uint32_t)tid - r * wI;
            const uint32_t dr = (uint32_t)L8_THREADS / wI, dc = (uint32_t)L8_THREADS - dr * wI;
            const int32_t n = (int32_t)nC;
            for (uint32_t e0 = tid; e0 < nInt; e0 += (uint32_t)L8_THREADS * U) {
                const int32_t *at[U];
                float p[U];
#pragma unroll
                for (int k = 0; k < U; k++) {
                    const bool in = e0 + (uint32_t)L8_THREADS * k < nInt;
                    at[k] = v + (in ? (size_t)(r + 2u) * nC + c + 2u : (size_t)2u * nC + 2u);      // a harmless cell for the idle slots
                    r += dr;
                    c += dc;
                    if (c >= wI) { c -= wI; r++; }
                }
#pragma unroll
                for (int k = 0; k < U; k++) {
                    float q = u[0] * (float)at[k][-1];
                    q = q + u[1] * (float)at[k][-n - 1];
                    q = q + u[2] * (float)at[k][-n];
                    q = q + u[3] * (float)at[k][-2];
                    q = q + u[4] * (float)at[k][-n - 2];
                    q = q + u[5] * (float)at[k][-2 * n - 2];
                    q = q + u[6] * (float)at[k][-2 * n - 1];
                    q = q + u[7] * (float)at[k][-2 * n];
                    p[k] = q;
                }
#pragma unroll
                for (int k = 0; k < U; k++) {
                    const uint32_t e = e0 + (uint32_t)L8_THREADS * k;
                    if (e < nInt) res[nInit + e] = (int32_t)((uint32_t)at[k][0] - (uint32_t)lsop8_estimate(p[k]));
                }
            }
        }
        if (tid == 0) a.status[t] = GF_K_OK;
    }
}

// ------------------------------------------------------------------------------------------------
// k_lsop8_pack: LsEncoder08.encode :113-134, the container of type 0.  Header (LsHeader.packHeader with 8 coefficients: 47 bytes),
// then HuffmanEncoder.encode (compress/HuffmanEncoder.java:124-219) of the initialisers' M32 bytes and of the interior's, into one
// bit store: the second segment's tree starts at the bit behind the first segment's last code.  The packing is zeroed up to its
// last byte first (the pad bits are zero) and then filled by OR: header bytes, the trees' leaf records, the codes.
//   * wave 0 builds the first segment's tree, wave 1 the second one's (huff_build.h: the reference's tree node for node);
//   * the text goes out a chunk of 1,024 values at a time: a thread strings the codes of four consecutive values together, a
//     workgroup scan places the strings, they meet in an LDS window that is flushed with whole-word stores (the two words a chunk
//     shares with its neighbours by OR).  A chunk whose codes do not fit the window is ORed into the packing directly.
// ------------------------------------------------------------------------------------------------
struct GfLsop8PackArgs {
    const int32_t *residuals;
    size_t resStride;
    const uint32_t *coefs;
    const int32_t *inStatus;   // k_lsop8_predict's: tiles with a status other than GF_K_OK get it and length 0
    uint8_t *out;              // slots of slotStride bytes, 16-byte aligned
    size_t slotStride;
    uint32_t *lengths;
    int32_t *status;
    size_t nTiles;
    uint32_t nInit, nInt;
    int codecIndex;
};
constexpr uint32_t P8_HEADER_BYTES = 47;
constexpr uint32_t P8_VPT = 4;                                  // values per thread and chunk
constexpr uint32_t P8_WIN_WORDS = 2048;                         // the window: 64 bits per value of a chunk
constexpr uint32_t P8_HIST_R = L8_THREADS / 64;                 // histogram replicas: one per wave

struct Lsop8PackShared {
    GfHuffTree T[2];
    uint64_t tab[2][256];          // (length << 56) | code of a byte
    uint32_t hist[P8_HIST_R][2][256];
    uint32_t win[P8_WIN_WORDS + 4];
    uint32_t waveSum[L8_THREADS / 64];
    uint32_t n[2], nM32[2], maxLen[2];
    unsigned long long textBits[2];
};

// nbits (<= 64) of x into the bit store at bit pos, by OR (atomic: neighbours share words)
__device__ __forceinline__ void p8_or_bits(uint32_t *words, uint32_t pos, uint64_t x, uint32_t nbits)
{
    if (nbits == 0u) return;
    const uint32_t s = pos & 31u, w = pos >> 5;
    atomicOr(&words[w], (uint32_t)(x << s));
    if (s + nbits > 32u) atomicOr(&words[w + 1u], s ? (uint32_t)(x >> (32u - s)) : (uint32_t)(x >> 32));
    if (s + nbits > 64u) atomicOr(&words[w + 2u], (uint32_t)(x >> (64u - s)));
}

__global__ __launch_bounds__(L8_THREADS) void k_lsop8_pack(GfLsop8PackArgs a)
{
    __shared__ Lsop8PackShared S;
    const int tid = threadIdx.x, lane = tid & 63, wave = (int)gf_wave_id();

    for (size_t t = blockIdx.x; t < a.nTiles; t += gridDim.x) {
        __syncthreads();                                       // (the tile before is done with S)
        const int32_t in = a.inStatus[t];
        if (in != GF_K_OK) {
            if (tid == 0) { a.status[t] = in; a.lengths[t] = 0; }
            continue;
        }
        const int32_t *__restrict__ res = a.residuals + t * a.resStride;
        uint32_t *out32 = reinterpret_cast<uint32_t *>(a.out + t * a.slotStride);

        // ---- the two histograms of M32 bytes ----
        for (uint32_t i = tid; i < P8_HIST_R * 2u * 256u; i += L8_THREADS) (&S.hist[0][0][0])[i] = 0u;
        __syncthreads();
        for (uint32_t i = tid; i < a.nInit + a.nInt; i += L8_THREADS) {
            const uint32_t x = (uint32_t)res[i];
            const int n = gf_m32_len(x);
            uint32_t *h = S.hist[wave][i < a.nInit ? 0 : 1];
            for (int b = 0; b < n; b++) atomicAdd(&h[gf_m32_byte(x, n, b)], 1u);
        }
        __syncthreads();

        // ---- the two trees: wave 0 the initialisers', wave 1 the interior's ----
        if (wave < 2) {
            const int g = wave;
            GfHuffTree &T = S.T[g];
            uint32_t *ccnt = &T.cnt[255];                      // compacted counts (the branch area is free until the merge)
            uint16_t *csym = T.bq;                             // compacted symbols
            int n = 0;
            uint32_t nM32 = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int s = lane + 64 * j;
                uint32_t cnt = 0;
#pragma unroll
                for (uint32_t r = 0; r < P8_HIST_R; r++) cnt += S.hist[r][g][s];
                const unsigned long long mk = __ballot(cnt != 0);
                const int pos = n + __popcll(mk & ((1ull << lane) - 1ull));
                if (cnt != 0) { ccnt[pos] = cnt; csym[pos] = (uint16_t)s; }
                n += __popcll(mk);
                nM32 += cnt;
            }
            __builtin_amdgcn_wave_barrier();
            // leaves in (count, symbol) order: a rank sort
            uint32_t rk[4], myc[4];
            uint16_t mys[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int i = lane + 64 * j;
                rk[j] = 0;
                myc[j] = 0;
                mys[j] = 0;
                if (i < n) {
                    const uint32_t ci = ccnt[i];
                    myc[j] = ci;
                    mys[j] = csym[i];
                    uint32_t rank = 0;
                    for (int q = 0; q < n; q++) {
                        const uint32_t cq = ccnt[q];
                        rank += (cq < ci || (cq == ci && q < i)) ? 1u : 0u;
                    }
                    rk[j] = rank;
                }
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int i = lane + 64 * j;
                if (i < n) { T.cnt[rk[j]] = myc[j]; T.sym[rk[j]] = (uint8_t)mys[j]; }
            }
            if (lane == 0) T.n = n;
            __builtin_amdgcn_wave_barrier();
            if (lane == 0 && n > 1) gf_huff_merge_t<false>(T, n, true);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) nM32 += gf_lane_xor(nM32, d);
            // codes; the leaves keep the place of their record in the serialised tree in nl[] (the merge is done with it)
            unsigned long long textBits = 0;
            uint32_t maxLen = 0;
            if (n == 1) {
                if (lane == 0) { S.tab[g][T.sym[0]] = 0; T.nl[0] = 0; }          // HuffmanEncoder.java:147-157: no text at all
            } else {
                uint32_t pos4[4];
                int len4[4];
                uint64_t code4[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int i = lane + 64 * j;
                    len4[j] = 0;
                    if (i < n) len4[j] = gf_huff_leaf_code(T, i, &code4[j], &pos4[j]);
                }
                __builtin_amdgcn_wave_barrier();                                  // (every walk read nl[] before a record place lands there)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int i = lane + 64 * j;
                    if (i < n) {
                        S.tab[g][T.sym[i]] = ((uint64_t)len4[j] << 56) | code4[j];
                        textBits += (unsigned long long)T.cnt[i] * (unsigned)len4[j];
                        maxLen = max(maxLen, (uint32_t)len4[j]);
                        T.nl[i] = (uint16_t)pos4[j];
                    }
                }
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                textBits += __shfl_xor(textBits, d, 64);
                maxLen = max(maxLen, gf_lane_xor(maxLen, d));
            }
            if (lane == 0) { S.n[g] = (uint32_t)n; S.nM32[g] = nM32; S.textBits[g] = textBits; S.maxLen[g] = maxLen; }
        }
        __syncthreads();

        // ---- the layout: where the segments begin and end ----
        unsigned long long segStart[2], treeBits[2];
        for (int g = 0; g < 2; g++) treeBits[g] = S.n[g] == 1u ? 17ull : 8ull + 10ull * S.n[g] - 1ull;
        segStart[0] = 8ull * P8_HEADER_BYTES;
        segStart[1] = segStart[0] + treeBits[0] + S.textBits[0];
        const unsigned long long totalBits = segStart[1] + treeBits[1] + S.textBits[1];
        const unsigned long long totalBytes = (totalBits + 7ull) >> 3;
        // (a code longer than 56 bits needs more values than a tile the entry points accept can hold)
        if (totalBytes > a.slotStride || totalBytes > 0x1fffffffull || S.maxLen[0] > 56u || S.maxLen[1] > 56u) {
            if (tid == 0) {
                a.status[t] = totalBytes > a.slotStride && totalBytes <= 0x1fffffffull ? GF_K_OVERFLOW : GF_K_ERR_UNSUPPORTED;
                a.lengths[t] = totalBytes <= 0xffffffffull ? (uint32_t)totalBytes : 0u;
            }
            continue;
        }
        const uint32_t nWords = (uint32_t)((totalBytes + 3ull) >> 2);
        for (uint32_t i = tid; i < nWords; i += L8_THREADS) out32[i] = 0u;
        __syncthreads();

        // ---- header and trees ----
        if (tid < (int)P8_HEADER_BYTES) {
            const uint32_t *cf = a.coefs + t * 16;
            uint32_t b;
            if (tid == 0) b = (uint32_t)a.codecIndex & 0xffu;
            else if (tid == 1) b = 0x40u;                          // COMPRESSION_TYPE_HUFFMAN | REVISION_FLAG
            else if (tid == 2) b = 8u;
            else if (tid < 39) b = (cf[(tid - 3) >> 2] >> (8 * ((tid - 3) & 3))) & 0xffu;      // seed, 8 floats
            else b = (S.nM32[(tid - 39) >> 2] >> (8 * ((tid - 39) & 3))) & 0xffu;              // the two M32 byte counts
            atomicOr(&out32[tid >> 2], b << (8 * (tid & 3)));
        }
        for (int g = 0; g < 2; g++) {
            const GfHuffTree &T = S.T[g];
            const uint32_t n = S.n[g], at = (uint32_t)segStart[g];
            if (tid == 0 && n > 1u) p8_or_bits(out32, at, n - 1u, 8);         // (the single-symbol form begins with eight zero bits)
            for (uint32_t i = tid; i < n; i += L8_THREADS)
                p8_or_bits(out32, at + 8u + T.nl[i], 1u | ((uint32_t)T.sym[i] << 1), 9);
        }

        // ---- the two texts ----
        for (int g = 0; g < 2; g++) {
            if (S.n[g] == 1u) continue;
            const int32_t *__restrict__ vals = res + (g ? a.nInit : 0u);
            const uint32_t nv = g ? a.nInt : a.nInit;
            const uint64_t *tab = S.tab[g];
            uint32_t running = (uint32_t)(segStart[g] + treeBits[g]);
            for (uint32_t c0 = 0; c0 < nv; c0 += L8_THREADS * P8_VPT) {
                const uint32_t i0 = c0 + (uint32_t)tid * P8_VPT;
                uint32_t x[P8_VPT], myBits = 0;
                int nb[P8_VPT];
#pragma unroll
                for (uint32_t k = 0; k < P8_VPT; k++) {
                    nb[k] = 0;
                    x[k] = 0;
                    if (i0 + k < nv) {
                        x[k] = (uint32_t)vals[i0 + k];
                        nb[k] = gf_m32_len(x[k]);
                        for (int b = 0; b < nb[k]; b++) myBits += (uint32_t)(tab[gf_m32_byte(x[k], nb[k], b)] >> 56);
                    }
                }
                // where the thread's string begins: a scan over the workgroup
                const uint32_t incl = gf_wave_incl_scan(myBits);
                if (lane == 63) S.waveSum[wave] = incl;
                __syncthreads();
                uint32_t before = 0, chunkBits = 0;
#pragma unroll
                for (int w = 0; w < L8_THREADS / 64; w++) {
                    const uint32_t ws = S.waveSum[w];
                    before += w < wave ? ws : 0u;
                    chunkBits += ws;
                }
                const uint32_t lead = running & 31u;
                const bool inWindow = lead + chunkBits <= P8_WIN_WORDS * 32u;
                const uint32_t winWords = (lead + chunkBits + 31u) >> 5;
                if (inWindow) {
                    for (uint32_t i = tid; i < winWords; i += L8_THREADS) S.win[i] = 0u;
                    __syncthreads();
                }
                uint32_t *words = inWindow ? S.win : out32;
                uint32_t pos = (inWindow ? lead : running) + before + incl - myBits;
                uint64_t str = 0;
                uint32_t strBits = 0;
#pragma unroll
                for (uint32_t k = 0; k < P8_VPT; k++) {
                    for (int b = 0; b < nb[k]; b++) {
                        const uint64_t e = tab[gf_m32_byte(x[k], nb[k], b)];
                        const uint32_t len = (uint32_t)(e >> 56);
                        if (strBits + len > 64u) {
                            p8_or_bits(words, pos, str, strBits);
                            pos += strBits;
                            str = 0;
                            strBits = 0;
                        }
                        str |= (e & 0x00ffffffffffffffull) << strBits;
                        strBits += len;
                    }
                }
                p8_or_bits(words, pos, str, strBits);
                __syncthreads();
                if (inWindow) {
                    uint32_t *dst = out32 + (running >> 5);
                    for (uint32_t i = tid; i < winWords; i += L8_THREADS) {
                        const uint32_t w = S.win[i];
                        if (i == 0u || i + 1u == winWords) atomicOr(&dst[i], w);
                        else dst[i] = w;
                    }
                    __syncthreads();
                }
                running += chunkBits;
            }
        }
        if (tid == 0) { a.status[t] = GF_K_OK; a.lengths[t] = (uint32_t)totalBytes; }
    }
}

// ------------------------------------------------------------------------------------------------
// k_lsop8_reconstruct: LsDecoder08.unpackInitializers + unpackInterior (:118-163), a tile per wave.
//
// Rows 0 and 1 and, band by band, columns 0 and 1 are prefix sums.  The interior is walked in bands of 64 rows, a lane per row; lane l
// is ONE column behind lane l - 1 (step s: lane l works on column c = s - l, columns 0 and 1 included: there the "computed" value is
// the border value, so that every row looks the same to the row below).  The neighbourhood lives in registers as float32 -- the
// reference converts each neighbour from int once per term, which gives the same float every time --: a lane keeps its own two
// previous values and columns c-2 .. c of the row above (A) and of the row two above (B).  The value entering A is what lane l - 1
// produced in the step before, the value entering B is the newest of lane l - 1's own A window: one DPP wave_shr:1 each.  Lane 0
// takes both from two full rows in LDS, which rows 0 and 1 fill first and lanes 62 and 63 of a band fill for the next one (a lane
// writes column s - 63 while lane 0 reads column s).  The per-cell dependent chain is the multiply by the newest cell, seven
// additions, the + 0.5f, the conversion and the residual's addition.  Residuals are fetched eight steps ahead of their use.
// ------------------------------------------------------------------------------------------------
struct GfLsop8ReconArgs {
    const int32_t *residuals;
    size_t resStride;
    const uint32_t *coefs;
    const int32_t *inStatus;   // may be null; tiles with a status other than GF_K_OK are skipped and keep it
    int32_t *values;
    int32_t *status;
    size_t nTiles;
    int nRows, nCols;
};
constexpr uint32_t R8_BLOCK = 8;                               // steps per block of the wavefront

__device__ __forceinline__ float lsop8_from_lane_above(float lane0Value, float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lane0Value), __float_as_int(x), 0x138, 0xf, 0xf, false));   // wave_shr:1
}

__global__ __launch_bounds__(64) void k_lsop8_reconstruct(GfLsop8ReconArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t r8Seam[];      // [2][nC]: the row above the band, the row two above
    const uint32_t lane = threadIdx.x;
    const uint32_t nR = (uint32_t)a.nRows, nC = (uint32_t)a.nCols, nCells = nR * nC;
    const uint32_t nInit = lsop8_n_init(nR, nC), wI = nC - 2u;
    uint32_t *seamA = r8Seam, *seamB = r8Seam + nC;

    for (size_t t = blockIdx.x; t < a.nTiles; t += gridDim.x) {
        if (a.inStatus && a.inStatus[t] != GF_K_OK) {
            if (lane == 0) a.status[t] = a.inStatus[t];
            continue;
        }
        const int32_t *__restrict__ res = a.residuals + t * a.resStride;
        const int32_t *__restrict__ inter = res + nInit;
        int32_t *__restrict__ v = a.values + t * (size_t)nCells;
        const uint32_t *cf = a.coefs + t * 16;
        const uint32_t seed = cf[0];
        float u[8];
#pragma unroll
        for (int i = 0; i < 8; i++) u[i] = __uint_as_float(cf[1 + i]);
        __syncthreads();                                       // (the tile before is done with the two rows)

        // row 0: the seed, then left differences; row 1: nC left differences, the first against the seed
        {
            uint32_t carry = seed;
            if (lane == 0) { v[0] = (int32_t)seed; seamB[0] = seed; }
            for (uint32_t c0 = 1; c0 < nC; c0 += 64) {
                const uint32_t c = c0 + lane;
                const uint32_t x = c < nC ? (uint32_t)res[c - 1u] : 0u;
                const uint32_t incl = gf_wave_incl_scan(x) + carry;
                if (c < nC) { v[c] = (int32_t)incl; seamB[c] = incl; }
                carry = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            }
            carry = seed;
            for (uint32_t c0 = 0; c0 < nC; c0 += 64) {
                const uint32_t c = c0 + lane;
                const uint32_t x = c < nC ? (uint32_t)res[nC - 1u + c] : 0u;
                const uint32_t incl = gf_wave_incl_scan(x) + carry;
                if (c < nC) { v[nC + c] = (int32_t)incl; seamA[c] = incl; }
                carry = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            }
        }
        uint32_t col0 = seed + (uint32_t)res[nC - 1u];           // column 0 of the row above the band: row 1's
        const uint32_t base2 = 2u * nC - 1u;
        for (uint32_t rb = 2; rb < nR; rb += 64) {
            __syncthreads();                                   // the two rows above the band are in LDS
            const uint32_t r = rb + lane;
            const bool rowIn = r < nR;
            const uint32_t rowsInBand = min(64u, nR - rb);
            // columns 0 and 1 of the band's rows
            const uint32_t x0 = rowIn ? (uint32_t)res[base2 + 2u * (r - 2u)] : 0u, x1 = rowIn ? (uint32_t)res[base2 + 2u * (r - 2u) + 1u] : 0u;
            const uint32_t b0 = gf_wave_incl_scan(x0) + col0, b1 = b0 + x1;
            col0 = (uint32_t)__builtin_amdgcn_readlane((int)b0, 63);
            const int32_t *__restrict__ myRes = inter + (size_t)(rowIn ? r - 2u : 0u) * wI;
            int32_t *__restrict__ myRow = v + (size_t)(rowIn ? r : 0u) * nC;

            float o1 = 0.f, o2 = 0.f, A0 = 0.f, A1 = 0.f, A2 = 0.f, B0 = 0.f, B1 = 0.f, B2 = 0.f;
            const uint32_t nSteps = nC + rowsInBand - 1u;
            int32_t rr[R8_BLOCK];
            // (a block's eight residuals and eight values are 32 contiguous bytes of the lane's row: two 16-byte accesses where the
            // whole block lies inside the row, single ones at its two ends)
            auto fetch = [&](uint32_t s0) {
                const int32_t c0 = (int32_t)s0 - (int32_t)lane;
                if (rowIn && c0 >= 2 && c0 + (int32_t)R8_BLOCK <= (int32_t)nC) {
                    const GfU4 lo = *reinterpret_cast<const GfU4 *>(myRes + (c0 - 2)), hi = *reinterpret_cast<const GfU4 *>(myRes + (c0 + 2));
                    rr[0] = (int32_t)lo.x; rr[1] = (int32_t)lo.y; rr[2] = (int32_t)lo.z; rr[3] = (int32_t)lo.w;
                    rr[4] = (int32_t)hi.x; rr[5] = (int32_t)hi.y; rr[6] = (int32_t)hi.z; rr[7] = (int32_t)hi.w;
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < R8_BLOCK; k++) {
                        const int32_t c = c0 + (int32_t)k;
                        rr[k] = rowIn && c >= 2 && c < (int32_t)nC ? myRes[c - 2] : 0;
                    }
                }
            };
            static_assert(R8_BLOCK == 8, "a block is two 16-byte accesses");
            fetch(0);
            for (uint32_t s0 = 0; s0 < nSteps; s0 += R8_BLOCK) {
                int32_t cur[R8_BLOCK];
                float sa[R8_BLOCK], sb[R8_BLOCK];
#pragma unroll
                for (uint32_t k = 0; k < R8_BLOCK; k++) {
                    cur[k] = rr[k];
                    const uint32_t cs = min(s0 + k, nC - 1u);                  // lane 0's column
                    sa[k] = (float)(int32_t)seamA[cs];
                    sb[k] = (float)(int32_t)seamB[cs];
                }
                fetch(s0 + R8_BLOCK);                                          // the next block's residuals, on their way while this one runs
                uint32_t outv[R8_BLOCK];
#pragma unroll
                for (uint32_t k = 0; k < R8_BLOCK; k++) {
                    const int32_t c = (int32_t)(s0 + k) - (int32_t)lane;
                    const bool active = rowIn && c >= 0 && c < (int32_t)nC;
                    const float bIn = lsop8_from_lane_above(sb[k], A0);
                    const float aIn = lsop8_from_lane_above(sa[k], o1);
                    B2 = B1; B1 = B0; B0 = bIn;
                    A2 = A1; A1 = A0; A0 = aIn;
                    float p = u[0] * o1;
                    p = p + u[1] * A1;
                    p = p + u[2] * A0;
                    p = p + u[3] * o2;
                    p = p + u[4] * A2;
                    p = p + u[5] * B2;
                    p = p + u[6] * B1;
                    p = p + u[7] * B0;
                    const uint32_t val = c == 0 ? b0 : c == 1 ? b1 : (uint32_t)lsop8_estimate(p) + (uint32_t)cur[k];
                    outv[k] = val;
                    if (active) { o2 = o1; o1 = (float)(int32_t)val; }
                }
                const int32_t c0 = (int32_t)s0 - (int32_t)lane;
                if (rowIn && c0 >= 0 && c0 + (int32_t)R8_BLOCK <= (int32_t)nC) {
                    *reinterpret_cast<GfU4 *>(myRow + c0) = GfU4{outv[0], outv[1], outv[2], outv[3]};
                    *reinterpret_cast<GfU4 *>(myRow + c0 + 4) = GfU4{outv[4], outv[5], outv[6], outv[7]};
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < R8_BLOCK; k++) {
                        const int32_t c = c0 + (int32_t)k;
                        if (rowIn && c >= 0 && c < (int32_t)nC) myRow[c] = (int32_t)outv[k];
                    }
                }
                if (lane >= 62u) {                                             // the rows above the next band (columns lane 0 has long passed)
                    uint32_t *seam = lane == 63u ? seamA : seamB;
#pragma unroll
                    for (uint32_t k = 0; k < R8_BLOCK; k++) {
                        const int32_t c = c0 + (int32_t)k;
                        if (rowIn && c >= 0 && c < (int32_t)nC) seam[c] = outv[k];
                    }
                }
            }
        }
        if (lane == 0) a.status[t] = GF_K_OK;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// launchers.  The three kernels walk the batch with a grid of at most GF_LSOP8_GRID_CAP workgroups.
// ------------------------------------------------------------------------------------------------
static unsigned lsop8_grid(size_t nTiles) { return (unsigned)(nTiles < GF_LSOP8_GRID_CAP ? nTiles : GF_LSOP8_GRID_CAP); }

hipError_t gf_launch_lsop8_predict(const int32_t *values, int32_t *residuals, size_t resStride, uint32_t *coefs, int32_t *status,
                                   size_t nTiles, int nRows, int nCols, hipStream_t stream)
{
    if (nTiles == 0) return hipSuccess;
    GfLsop8PredictArgs a{values, residuals, resStride, coefs, status, nTiles, nRows, nCols};
    hipLaunchKernelGGL(k_lsop8_predict, dim3(lsop8_grid(nTiles)), dim3(L8_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_lsop8_pack(const int32_t *residuals, size_t resStride, const uint32_t *coefs, const int32_t *inStatus, uint8_t *out,
                                size_t slotStride, uint32_t *lengths, int32_t *status, size_t nTiles, int nRows, int nCols, int codecIndex,
                                hipStream_t stream)
{
    if (nTiles == 0) return hipSuccess;
    GfLsop8PackArgs a{residuals, resStride, coefs, inStatus, out, slotStride, lengths, status, nTiles,
                      (uint32_t)(2 * nRows + 2 * nCols - 5), (uint32_t)(nRows - 2) * (uint32_t)(nCols - 2), codecIndex};
    hipLaunchKernelGGL(k_lsop8_pack, dim3(lsop8_grid(nTiles)), dim3(L8_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t gf_launch_lsop8_reconstruct(const int32_t *residuals, size_t resStride, const uint32_t *coefs, const int32_t *inStatus,
                                       int32_t *values, int32_t *status, size_t nTiles, int nRows, int nCols, hipStream_t stream)
{
    if (nTiles == 0) return hipSuccess;
    const size_t dyn = (size_t)2 * (size_t)nCols * 4;          // (nCols <= GF_LSOP8_MAX_COLS: the entry points refuse wider tiles)
    static GfDynLdsOptIn opt;
    const hipError_t e = gf_opt_in_dyn_lds(k_lsop8_reconstruct, dyn, opt);
    if (e != hipSuccess) return e;
    GfLsop8ReconArgs a{residuals, resStride, coefs, inStatus, values, status, nTiles, nRows, nCols};
    hipLaunchKernelGGL(k_lsop8_reconstruct, dim3(lsop8_grid(nTiles)), dim3(64), dyn, stream, a);
    return hipGetLastError();
}
