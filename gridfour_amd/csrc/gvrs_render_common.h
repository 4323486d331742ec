// gvrs_render_common.h -- a value turned into an ARGB word, restated once for host and device: the colour palette lookup
// (imaging/palette/ColorPaletteTable.java:395-456 getArgb, :481-541 getArgbWithShade, :567-598 the UnlimitedRange forms;
// ColorPaletteRecordRGB.java:96-121; ColorPaletteRecordHSV.java:146-194; java.util.Arrays.binarySearch(double[], double) and
// java.awt.Color.HSBtoRGB as the JDK defines them) and the illumination model of the reference's demos
// (demo/src/main/java/org/gridfour/demo/globalDEM/ExtractData.java:405-415, demo/geoTiff/DemoCOG.java:421-431).  Used by the
// kernels of gvrs_render.hip, by the palette packer of gvrs_api_render.hip and by a stand-alone CPU harness
// (tests/csrc/render_harness.cpp).
//
// THE ARITHMETIC IS THE CONTRACT, as in gvrs_interp_common.h: the reference's operands, order and association, one rounding per
// operation (-ffp-contract=off, no fma), plain / and sqrt, Java's conversions.  The palette records' part is double, HSBtoRGB is
// float32.  Reference paths are relative to core/src/main/java/org/gridfour/ unless they begin with demo/.
#pragma once

#include <math.h>
#include <stdint.h>

#include "gvrs_interp_common.h"

#define GF_PAL_RGB 0
#define GF_PAL_HSV 1
#define GF_PAL_MAX_RECORDS 256
#define GF_RENDER_ELEM_Z 4                          // the cells form's fifth input: doubles, looked up as they are

// One record as the kernels read it (72 bytes).  RGB: c0 = r0, g0, b0 and d = deltaR, deltaG, deltaB, integers held as doubles
// (ColorPaletteRecordRGB.java:76-84); HSV: c0 = h0, s0, v0 and d = deltaH, deltaS, deltaV with the constructor's rules applied
// (ColorPaletteRecordHSV.java:98-125).
struct GfPalRec {
    double range0, range1;
    double c0[3], d[3];
    int32_t model, wrapAround;
};

// The table's scalars (64 bytes).  A packed table is GfPalHead | double keys[n] | GfPalRec recs[n], records sorted, keys[i] =
// recs[i].range0 (ColorPaletteTable.java:206-210).
struct GfPalHead {
    int32_t n;
    uint32_t argbForNull;
    int32_t normalized, hinge, hingeIndex, pad;
    double rangeMin, rangeMax;                      // records[0].range0, records[n - 1].range1 (:234-235)
    double normMin, normMax, hingeValue;            // normalizedRangeMin / Max, hingeValue
};

// the illumination model's constants, from the caller
struct GfRenderLight {
    double xGain, yGain;
    double sun[3];
    double ambient;
};

GF_HD int32_t gf_render_java_int(double x) { return gf_interp_java_int(x); }

// Java's (int) of a float: NaN -> 0, saturating
GF_HD int32_t gf_render_java_int_f(float x)
{
    if (x != x) return 0;
    if (x >= 2147483648.0f) return 2147483647;
    if (x <= -2147483648.0f) return (int32_t)0x80000000u;
    return (int32_t)x;
}

// Double.doubleToLongBits: every NaN is 0x7ff8000000000000
GF_HD int64_t gf_render_double_bits(double x)
{
    if (x != x) return (int64_t)0x7ff8000000000000ll;
    union { double d; int64_t i; } b;
    b.d = x;
    return b.i;
}

// java.util.Arrays.binarySearch(double[] a, double key) as the JDK writes it (binarySearch0): with equal keys the index found
// depends on the probes, -0.0 sorts below 0.0 and NaN above everything
GF_HD int32_t gf_render_binary_search(const double *keys, int32_t n, double key)
{
    int32_t low = 0, high = n - 1;
    while (low <= high) {
        const int32_t mid = (int32_t)(((uint32_t)low + (uint32_t)high) >> 1);
        const double midVal = keys[mid];
        if (midVal < key) low = mid + 1;
        else if (midVal > key) high = mid - 1;
        else {
            const int64_t midBits = gf_render_double_bits(midVal), keyBits = gf_render_double_bits(key);
            if (midBits == keyBits) return mid;
            if (midBits < keyBits) low = mid + 1;
            else high = mid - 1;
        }
    }
    return -(low + 1);
}

// java.awt.Color.HSBtoRGB(float, float, float); (float) Math.floor(x) of a float x is floorf(x)
GF_HD uint32_t gf_render_hsb_to_rgb(float hue, float saturation, float brightness)
{
    int32_t r = 0, g = 0, b = 0;
    if (saturation == 0) {
        r = g = b = gf_render_java_int_f(brightness * 255.0f + 0.5f);
    } else {
        const float h = (hue - floorf(hue)) * 6.0f;
        const float f = h - floorf(h);
        const float p = brightness * (1.0f - saturation);
        const float q = brightness * (1.0f - saturation * f);
        const float t = brightness * (1.0f - (saturation * (1.0f - f)));
        float fr = 0, fg = 0, fb = 0;
        bool hit = true;
        switch (gf_render_java_int_f(h)) {
        case 0: fr = brightness, fg = t, fb = p; break;
        case 1: fr = q, fg = brightness, fb = p; break;
        case 2: fr = p, fg = brightness, fb = t; break;
        case 3: fr = p, fg = q, fb = brightness; break;
        case 4: fr = t, fg = p, fb = brightness; break;
        case 5: fr = brightness, fg = p, fb = q; break;
        default: hit = false; break;
        }
        if (hit) {
            r = gf_render_java_int_f(fr * 255.0f + 0.5f);
            g = gf_render_java_int_f(fg * 255.0f + 0.5f);
            b = gf_render_java_int_f(fb * 255.0f + 0.5f);
        }
    }
    return 0xff000000u | ((uint32_t)r << 16) | ((uint32_t)g << 8) | (uint32_t)b;
}

// a record's getArgb (withShade false) / getArgbWithShade: ColorPaletteRecordRGB.java:96-121, ColorPaletteRecordHSV.java:146-194.
// A NaN t (range0 == range1) passes both comparisons.
GF_HD uint32_t gf_render_record(const GfPalRec &rec, double z, double shade, bool withShade)
{
    double t = (z - rec.range0) / (rec.range1 - rec.range0);
    if (t < 0) t = 0;
    else if (t > 1) t = 1;
    if (rec.model == GF_PAL_RGB) {
        int32_t r, g, b;
        if (withShade) {
            r = gf_render_java_int(shade * (rec.d[0] * t + rec.c0[0]) + 0.5);
            g = gf_render_java_int(shade * (rec.d[1] * t + rec.c0[1]) + 0.5);
            b = gf_render_java_int(shade * (rec.d[2] * t + rec.c0[2]) + 0.5);
        } else {
            r = gf_render_java_int(rec.d[0] * t + rec.c0[0] + 0.5);
            g = gf_render_java_int(rec.d[1] * t + rec.c0[1] + 0.5);
            b = gf_render_java_int(rec.d[2] * t + rec.c0[2] + 0.5);
        }
        return 0xff000000u | ((uint32_t)r << 16) | ((uint32_t)g << 8) | (uint32_t)b;
    }
    double a = rec.d[0] * t + rec.c0[0];
    if (rec.wrapAround) {
        if (a < 0.0) a += 360.0;
        else if (a > 360.0) a -= 360.0;
    }
    const float s = (float)(rec.d[1] * t + rec.c0[1]);
    const float v = withShade ? (float)((rec.d[2] * t + rec.c0[2]) * shade) : (float)(rec.d[2] * t + rec.c0[2]);
    const float h = (float)(a / 360.0);
    return gf_render_hsb_to_rgb(h, s, v);
}

// ColorPaletteTable.getArgb / getArgbWithShade (:395-456, :481-541)
GF_HD uint32_t gf_render_lookup(const GfPalHead &p, const double *keys, const GfPalRec *recs, double zTarget, double shade, bool withShade)
{
    double z = zTarget;
    if (p.normalized) {
        if (p.hinge) {
            if (z < p.hingeValue) {
                const double t = (z - p.normMin) / (p.hingeValue - p.normMin);
                z = t * (recs[p.hingeIndex - 1].range1 - recs[0].range0) + recs[0].range0;
            } else {
                const double t = (z - p.hingeValue) / (p.normMax - p.hingeValue);
                z = t * (recs[p.n - 1].range1 - recs[p.hingeIndex].range0) + recs[p.hingeIndex].range0;
            }
        } else {
            const double t = (z - p.normMin) / (p.normMax - p.normMin);
            z = t * (recs[p.n - 1].range1 - recs[0].range0) + recs[0].range0;
        }
    }
    // (:423-455: an exact match asks its record; -1 is below the table; otherwise the record before the insertion point, when
    // its range1 reaches z.  One call of the record for both.)
    int32_t index = gf_render_binary_search(keys, p.n, z);
    if (index == -1) return p.argbForNull;
    const bool exact = index >= 0;
    if (!exact) index = -(index + 1) - 1;
    if (!exact && !(recs[index].range1 >= z)) return p.argbForNull;
    return gf_render_record(recs[index], z, shade, withShade);
}

// ... with unlimited: getArgbUnlimitedRange / getArgbUnlimitedRangeWithShade (:567-598)
GF_HD uint32_t gf_render_palette(const GfPalHead &p, const double *keys, const GfPalRec *recs, double z, double shade, bool withShade,
                                 bool unlimited)
{
    if (unlimited) {
        if (z < p.rangeMin) z = p.rangeMin;
        else if (z > p.rangeMax) z = p.rangeMax;
    }
    return gf_render_lookup(p, keys, recs, z, shade, withShade);
}

// the demos' illumination (demo/.../ExtractData.java:405-415, DemoCOG.java:421-431): the gains carry the sign and steepen
GF_HD double gf_render_shade(double zx, double zy, const GfRenderLight &l)
{
    double nx = zx * l.xGain;
    double ny = zy * l.yGain;
    const double s = sqrt(nx * nx + ny * ny + 1);
    nx /= s;
    ny /= s;
    const double nz = 1 / s;
    const double dot = nx * l.sun[0] + ny * l.sun[1] + nz * l.sun[2];
    double shade = l.ambient;
    if (dot > 0) shade = dot * (1 - l.ambient) + l.ambient;
    return shade;
}

// a cell of a block as a double z: what gf_interp_samples does with one cell
GF_HD double gf_render_cell_f32(uint32_t bits) { return gf_interp_sample_f32(bits); }
GF_HD double gf_render_cell_i32(int32_t cell, int32_t fill) { return gf_interp_sample_i32(cell, fill); }
