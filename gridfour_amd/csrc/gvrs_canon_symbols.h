// gvrs_canon_symbols.h -- the symbol set of Gridfour's canonical Huffman coder (compress/canonicalHuffman/
// CanonicalHuffman.java:74-80) and the classification of a value by countSymbols, shared by the encode side
// (gvrs_canon_common.h) and the decode side (gvrs_canon_decode_common.h, k_canon_stats).  Included inside the
// kernel file's anonymous namespace through those headers.
#pragma once

constexpr int CN_SYMS = 260;                     // CanonicalHuffman.java:74-80
constexpr int CN_NULL = 256;
constexpr int CN_ESC1 = 257;                     // one raw byte follows
constexpr int CN_ESC2 = 258;                     // two raw bits follow
constexpr int CN_EOT = 259;
constexpr int CN_META = 20;                      // LengthEncoder.SYMBOL_SET_SIZE + 1 (end-of-text)

// value -> (target symbol, escape kind) as CanonicalHuffman.countSymbols :352-418 classifies it.
// kind: 0 none, 1..3 = that many 2-bit escapes, 4..6 = 1..3 one-byte escapes, 7 = null symbol
__device__ __forceinline__ uint32_t cn_classify_count(uint32_t x, uint32_t *kind)
{
    const int32_t s = (int32_t)x;
    if (x + 128u < 256u) { *kind = 0; return x + 128u; }
    if (x + 512u < 1024u) { *kind = 1; return (uint32_t)((s >> 2) + 128); }
    if (x + 2048u < 4096u) { *kind = 2; return (uint32_t)((s >> 4) + 128); }
    if (x + 8192u < 16384u) { *kind = 3; return (uint32_t)((s >> 6) + 128); }
    if (x + 32768u < 65536u) { *kind = 4; return (uint32_t)((s >> 8) + 128); }
    if (x == GF_NULL_CODE) { *kind = 7; return (uint32_t)CN_NULL; }
    if (x + 8388608u < 16777216u) { *kind = 5; return (uint32_t)((s >> 16) + 128); }
    *kind = 6;
    return (uint32_t)((s >> 24) + 128);
}
