// gvrs_file_points_store.h -- THE STORE RULE of a cell, restated once for host and device: what TileElement*.setValue does to a value
// a user stores (gvrs/TileElementInt.java:118-126, TileElementShort.java:136-143, TileElementFloat.java:133-149,
// TileElementIntCodedFloat.java:152-169: the range check that throws, Float.equals for the fill, the float-to-code conversion)
// and what TileElement*.hasValidData asks of a tile's cell.  Used by the block write (k_block_cut_elems, gvrs_blocks_write.hip),
// by the writes at scattered points (k_points_claim, k_points_store, gvrs_file_points_write.hip) and by a stand-alone CPU program
// (tests/csrc/file_points_write_test.cpp).  A cell travels as its 32 bits (a SHORT's: the low 16); K is the element's kind, 0 INT,
// 1 SHORT, 2 FLOAT, 3 int-coded float (= GF_ELEM_* = GF_K_ELEM_*).  Built without contraction wherever it is built.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "gvrs_common.h"

constexpr int GF_STORE_INT = 0, GF_STORE_SHORT = 1, GF_STORE_FLOAT = 2, GF_STORE_ICF = 3;

// an element's constants (workgroup-uniform in the kernels)
struct GfStoreElem {
    uint32_t fill;             // the tile's fill cell (SHORT: 16 bits; ICF: the code fill_i)
    uint32_t fillF;            // ICF: fill_f's bits
    uint32_t lo, hi;           // the range: int32, or float bits
    float scale, offset;
    bool nanFill;              // FLOAT: the fill is a NaN; ICF: fill_f is
};

GF_HD float gf_store_float(uint32_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}

// fillBits: fill_i (SHORT: any upper bits are dropped; ICF: the code), or a FLOAT's fill_f as bits; fillFBits: an ICF's fill_f
GF_HD GfStoreElem gf_store_elem(int kind, uint32_t fillBits, uint32_t fillFBits, uint32_t minBits, uint32_t maxBits, float scale, float offset)
{
    GfStoreElem e;
    e.fill = kind == GF_STORE_SHORT ? fillBits & 0xffffu : fillBits;
    e.fillF = fillFBits;
    e.lo = minBits, e.hi = maxBits;
    e.scale = scale, e.offset = offset;
    const float f = gf_store_float(kind == GF_STORE_ICF ? fillFBits : fillBits);
    e.nanFill = f != f;
    return e;
}

// "this cell is data": TileElement*.hasValidData on the TILE's cell (an ICF's is its code)
template <int K>
GF_HD bool gf_store_valid(uint32_t o, const GfStoreElem &p)
{
    if (K == GF_STORE_FLOAT) {
        const float f = gf_store_float(o);
        return p.nanFill ? !(f != f) : f != gf_store_float(p.fill);            // (the float comparison: -0.0 is the fill 0.0, a NaN is data)
    }
    return o != p.fill;
}

// Float.equals: the bits, any NaN being one value
GF_HD bool gf_store_float_equals(uint32_t v, uint32_t fillBits, bool nanFill)
{
    const float f = gf_store_float(v);
    return v == fillBits || (nanFill && f != f);
}

// (int) Math.floor((double)((v - offset) * scale) + 0.5): subtraction and product rounded once each in float32, the sum and the floor
// in double, the cast saturating as Java's does (a NaN: 0)
GF_HD uint32_t gf_store_icf_code(float v, float scale, float offset)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const float d = __fmul_rn(__fsub_rn(v, offset), scale);
#else
    const float t = v - offset;
    const float d = t * scale;
#endif
    const double x = floor((double)d + 0.5);
    if (x != x) return 0u;
    if (x >= 2147483647.0) return 0x7fffffffu;
    if (x <= -2147483648.0) return 0x80000000u;
    return (uint32_t)(int32_t)x;
}

// setValue / setIntValue on one value v: true when the reference stores it and o is then the tile's cell; false when it throws (the
// value is out of range and is not the fill): o is v, or for an ICF the fill's code.
template <int K>
GF_HD bool gf_store_value(uint32_t v, const GfStoreElem &p, uint32_t &o)
{
    o = v;
    if (K == GF_STORE_INT) return ((int32_t)v >= (int32_t)p.lo && (int32_t)v <= (int32_t)p.hi) || v == p.fill;
    if (K == GF_STORE_SHORT) {
        const int32_t s = (int32_t)(int16_t)v;
        return (s >= (int32_t)p.lo && s <= (int32_t)p.hi) || v == p.fill;
    }
    const float f = gf_store_float(v);
    const bool inRange = gf_store_float(p.lo) <= f && f <= gf_store_float(p.hi);
    if (K == GF_STORE_FLOAT) return inRange || gf_store_float_equals(v, p.fill, p.nanFill);
    const bool isFill = gf_store_float_equals(v, p.fillF, p.nanFill);
    o = (isFill || !inRange) ? p.fill : gf_store_icf_code(f, p.scale, p.offset);
    return isFill || inRange;
}

// the same for a kind known only when it runs
GF_HD bool gf_store_value_of(int kind, uint32_t v, const GfStoreElem &p, uint32_t &o)
{
    switch (kind) {
    case GF_STORE_INT: return gf_store_value<GF_STORE_INT>(v, p, o);
    case GF_STORE_SHORT: return gf_store_value<GF_STORE_SHORT>(v, p, o);
    case GF_STORE_FLOAT: return gf_store_value<GF_STORE_FLOAT>(v, p, o);
    default: return gf_store_value<GF_STORE_ICF>(v, p, o);
    }
}
GF_HD bool gf_store_valid_of(int kind, uint32_t o, const GfStoreElem &p)
{
    return kind == GF_STORE_FLOAT ? gf_store_valid<GF_STORE_FLOAT>(o, p) : gf_store_valid<GF_STORE_INT>(o, p);
}
