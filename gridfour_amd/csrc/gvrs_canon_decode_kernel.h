// gvrs_canon_decode_kernel.h -- k_canon_decode, the CodecCanonHuffman decoder of gvrs_canon_decode.hip (see there for the
// reference lines and the phases), as a template on one switch:
//   k_canon_decode<false>  CodecCanonHuffman.decode -- gvrs_canon_decode.hip, both of its builds (256 and 512 threads)
//   k_canon_decode<true>   the text for CodecCanonHuffman.analyze (CodecCanonHuffman.java:217-271) -- gvrs_aux.hip, 256 threads:
//                          every packing that is not the uniform form goes out as it stands, up to nRows * nCols values in
//                          stream order and zeros behind the end-of-text symbol, at a tile stride of gf_canon_stats_stride()
//                          values; no predictor check, no phase 3.  k_canon_stats counts it.
// (The two live in different translation units: a second instantiation beside the first changed the register allocation of
// the decoder, 62 -> 64 VGPRs in the 256-thread build, although its code is the same.)
// Include inside the kernel file's anonymous namespace after gvrs_canon_decode_common.h.
#pragma once

template <bool ANALYZE>
__global__ __launch_bounds__(DEC_THREADS, DEC_THREADS == 256 ? 4 : 8) void k_canon_decode(GfDecodeArgs a)
{
    __shared__ CanonDec S;

    const int tid = threadIdx.x;
    const uint32_t nR = (uint32_t)a.nRows, nC = (uint32_t)a.nCols, nCells = nR * nC;
    const uint32_t *__restrict__ w32 = reinterpret_cast<const uint32_t *>(a.blob);
    const uint64_t nWords = (a.blobBytes + 3) >> 2;
    const uint32_t capWords = a.ldsTextBytes >> 2;
    // the byte stage of phase 2 (CdCellSink): the sync arrays qe / qc are dead by then, the rest sits behind the text copy
    // (one subsequence per thread: every thread has its start in a register before the first value is staged, so all four
    // sync arrays serve as stage; two per thread: the starts of the second half are still needed, qe / qc only)
    uint8_t *const stageA = reinterpret_cast<uint8_t *>(CD_NCUR == 1 ? S.qs : S.qe);
    const uint32_t stageCapA = (uint32_t)((CD_NCUR == 1 ? 4 : 2) * sizeof(S.qe));
    static_assert(offsetof(CanonDec, qe) == offsetof(CanonDec, qs) + sizeof(S.qs) && offsetof(CanonDec, qx) == offsetof(CanonDec, qc) + sizeof(S.qc),
                  "qs .. qx form one stretch of LDS");
    static_assert(offsetof(CanonDec, qc) == offsetof(CanonDec, qe) + sizeof(S.qe), "qe and qc form one stretch of LDS");

    // behind the canonical run of the fast legacy kernel (round 5; DEC_FAST_CANON in gvrs_decode.hip, a.retryFlag non-null): only the tiles
    // that run marked, and nothing at all when it marked none
    if (a.retryFlag && a.retryFlag[0] == 0u) return;

    GF_FOR_WG_TILE(t, a.nTiles) {                                         // no tile loop: see gvrs_kernels.h
        if (a.retryFlag && a.status[t] != (int32_t)GF_K_LEAN_RETRY) continue;
        const uint64_t off = a.offsets ? a.offsets[t] : (uint64_t)t * a.slotStride;
        const uint32_t len = a.lengths[t];
        uint32_t *o = reinterpret_cast<uint32_t *>(a.values) + t * (size_t)(ANALYZE ? gf_canon_stats_stride(nCells) : nCells);
        const uint8_t *__restrict__ pk = a.blob + off;

        if (len < 6 || off + len > a.blobBytes) {                 // packing[1..5] -> ArrayIndexOutOfBounds
            if (tid == 0) a.status[t] = GF_K_ERR_BOUNDS;
            __syncthreads();
            continue;
        }
        const int predictor = (int8_t)pk[1];
        const uint32_t seed = (uint32_t)pk[2] | ((uint32_t)pk[3] << 8) | ((uint32_t)pk[4] << 16) | ((uint32_t)pk[5] << 24);
        if (predictor == 0 && len == 6) {                         // uniform tile, CodecCanonHuffman.java:171-176 (analyze: :233-244, no text)
            if constexpr (!ANALYZE)
                for (uint32_t i = tid; i < nCells; i += DEC_THREADS) o[i] = seed;
            if (tid == 0) a.status[t] = GF_K_OK;
            __syncthreads();
            continue;
        }
        // (analyze never looks at the predictor byte before the text is decoded)
        if (!ANALYZE && (predictor < 1 || predictor > 4 || (predictor == 2 && nC < 2))) {   // :208-209 IOException; Linear output[1]
            if (tid == 0) a.status[t] = predictor < 1 || predictor > 4 ? GF_K_ERR_FORMAT : GF_K_ERR_BOUNDS;
            __syncthreads();
            continue;
        }
        const int model = ANALYZE ? 4 : predictor;                 // (model 4: the stream in cell order, nCells values)

        // the packing as words: aligned words of the blob, bit positions carry the misalignment
        const uint64_t word0 = off >> 2;
        const uint32_t bias = (uint32_t)(off & 3u) * 8u;
        const uint32_t endBit = bias + len * 8u;
        const uint32_t needWords = (endBit + 31u) / 32u + 4u;       // the readers look up to three words ahead
        const bool textInLds = needWords <= capWords;
        if (textInLds) cd_stage_text(w32, word0, nWords, endBit, needWords);
        const CdTextLds TL{needWords};
        const CdTextGlobal TG{w32 + word0, (uint32_t)min((uint64_t)needWords, nWords - word0)};   // huge packing: read in place
        __syncthreads();

        // ---------------- phases 0-2: the canonical-Huffman stream, values to their cells ----------------
        const uint32_t nStream = gf_stream_len(model, nR, nC);
        // Triangle tiles of the one-subsequence-per-thread build: the staged residuals become the tile in one go (cd_fused_triangle)
        // (the stage behind the sync arrays: what this packing leaves of the text buffer, then the bytes behind it)
        uint8_t *const stageB = reinterpret_cast<uint8_t *>(cdLdsText + (textInLds ? needWords : 0u));
        // (less the last word of part B where there is one: cd_fused_triangle reads the stage two words at a time, and the
        // word behind the last byte it may ask for has to lie inside the workgroup's LDS as well)
        const uint32_t stageBytesB = (capWords - (textInLds ? needWords : 0u)) * 4u + a.ldsStageBytes;
        const uint32_t stageCap = stageCapA + (stageBytesB >= 4u ? stageBytesB - 4u : 0u);
#ifdef GF_DIAG
        const bool fuse = !ANALYZE && cd_fuse_eligible(model, nR, nC, stageCap) && !(a.phaseLimit & 0x300);
        const CdCellSink sink{o, GfCellMap::make(model, nR, nC), nStream, !(a.phaseLimit & 0x100),
                              stageA, stageB, stageCapA, stageCap, 0u, fuse};
        uint32_t *stamps = a.debug ? a.debug + t * 16 : nullptr;
        if (stamps && tid == 0) stamps[0] = (uint32_t)__builtin_amdgcn_s_memtime();
#else
        const bool fuse = !ANALYZE && cd_fuse_eligible(model, nR, nC, stageCap);
        const CdCellSink sink{o, GfCellMap::make(model, nR, nC), nStream, true,
                              stageA, stageB, stageCapA, stageCap, 0u, fuse};
        constexpr uint32_t *stamps = nullptr;
#endif
        uint32_t endPos, nValues;
        const uint32_t *pre = a.trees ? a.trees + t * GF_CANON_REC_WORDS : nullptr;
        // the token table of the synchronisation pass: in the value stage behind the text, which is idle until phase 2
        uint16_t *const tok = a.ldsStageBytes >= (sizeof(uint16_t) << CD_LUT_BITS) ? reinterpret_cast<uint16_t *>(cdLdsText + capWords) : nullptr;
#ifdef GF_DIAG
        const int diagLimit = a.phaseLimit & 0xff;
#else
        constexpr int diagLimit = 0;
#endif
        const int32_t st = textInLds ? cd_decode_stream(S, TL, bias + 48u, endBit, nCells, nStream, sink, &endPos, &nValues, stamps, pre, bias, tok, diagLimit)
                                     : cd_decode_stream(S, TG, bias + 48u, endBit, nCells, nStream, sink, &endPos, &nValues, stamps, pre, bias);
        if (st != GF_K_OK) {
            if (tid == 0) a.status[t] = st;
            __syncthreads();
            continue;
        }

        // ---------------- phase 3: predictor inverse ----------------
        if constexpr (!ANALYZE) {
            if (fuse) cd_fused_triangle(S, sink, seed, nR, nC, o);
            else gf_predictor_inverse(model, seed, o, nR, nC, nullptr);
        }
#ifdef GF_DIAG
        if (stamps && tid == 0) stamps[6] = (uint32_t)__builtin_amdgcn_s_memtime();
#endif
        if (tid == 0) a.status[t] = GF_K_OK;
        __syncthreads();
    }
}
