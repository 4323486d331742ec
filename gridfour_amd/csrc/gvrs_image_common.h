// gvrs_image_common.h -- packed ARGB words and the element planes the reference stores them as, restated once for host and device:
// the channels of a word, the two plane models, the word joined from three planes, and the box average of packed pixels.  Used by
// the kernels of gvrs_image.hip and gvrs_downsample.hip and by a stand-alone CPU harness (tests/csrc/image_harness.cpp).
// Reference: demo/src/main/java/org/gridfour/demo/imaging/ExperimentalImageStorage.java:203-213 (elements r, g, b), :242-256 (Y, Co,
// Cg after the reversible YCoCg-R transform), :275-286 (the YCoCg planes read back into words);
// demo/src/main/java/org/gridfour/demo/geoTiff/DemoCOG.java:735-770 (makeReducedImage).
//
// THE ARITHMETIC IS THE CONTRACT: results are compared bit for bit.  Everything is Java's wrapping 32-bit int: the sums and left
// shifts are done on uint32_t, >> is the arithmetic shift of the int32_t.
//   SPLIT: r = (w >> 16) & 0xff, g = (w >> 8) & 0xff, b = w & 0xff; alpha is ignored.  GF_IMAGE_RGB: the planes are r, g, b.
//   GF_IMAGE_YCOCG: Co = r - b; tmp = b + (Co >> 1); Cg = g - tmp; Y = tmp + (Cg >> 1); the planes are Y, Co, Cg (Y in 0 .. 255, Co
//   and Cg in -255 .. 255: every plane value fits int16).
//   JOIN, of ANY three ints (planes may hold fill or damaged values): YCoCg first undoes the transform, tmp = Y - (Cg >> 1);
//   g = Cg + tmp; b = tmp - (Co >> 1); r = b + Co; then both models give word = (((0xff00 | r) << 8 | g) << 8) | b.  r, g and b are
//   NOT masked: bits above a channel's eight spill into the channels above it, and r's bits 8 .. 15 fall off the top.  The reference
//   has no read loop of its own for the elements r, g, b: the RGB join is its YCoCg loop without the transform.
//   By hand, every plane INT_MIN (the fill of an INT element): RGB: 0xff00 | r = 0x8000ff00, << 8 = 0x00ff0000, | g = 0x80ff0000,
//   << 8 = 0xff000000, | b = 0xff000000.  YCoCg: Cg >> 1 = -2^30, tmp = -2^31 + 2^30 = -2^30, g = -2^31 - 2^30 = 2^30 (wrapped),
//   b = -2^30 - (-2^30) = 0, r = INT_MIN; 0x00ff0000 | 2^30 = 0x40ff0000, << 8 = 0xff000000, | 0 = 0xff000000.
//   REDUCE, a window of f x f words, n = f * f: the channels are summed, c = (cSum + n / 2) / n (Java's int division; nothing is
//   negative), word = 0xff000000 | (r << 16) | (g << 8) | b.  f <= GF_IMAGE_MAX_FACTOR: 2899^2 * 255 + 2899^2 / 2 = 2,147,273,355
//   still fits an int and 2900^2 does not; beyond it the reference's sums wrap.
#pragma once

#include <stdint.h>

#include "gvrs_common.h"

#define GF_IMAGE_MODEL_RGB 0
#define GF_IMAGE_MODEL_YCOCG 1
#define GF_IMAGE_MAX_FACTOR 2899

GF_HD int32_t gf_img_sar1(uint32_t v) { return (int32_t)v >> 1; }

// the three plane values of a word
GF_HD void gf_img_split(int model, uint32_t w, int32_t p[3])
{
    const uint32_t r = (w >> 16) & 0xffu, g = (w >> 8) & 0xffu, b = w & 0xffu;
    if (model == GF_IMAGE_MODEL_RGB) {
        p[0] = (int32_t)r, p[1] = (int32_t)g, p[2] = (int32_t)b;
        return;
    }
    const uint32_t co = r - b;
    const uint32_t tmp = b + (uint32_t)gf_img_sar1(co);
    const uint32_t cg = g - tmp;
    const uint32_t y = tmp + (uint32_t)gf_img_sar1(cg);
    p[0] = (int32_t)y, p[1] = (int32_t)co, p[2] = (int32_t)cg;
}

// the word of three plane values, whatever they are
GF_HD uint32_t gf_img_join(int model, int32_t p0, int32_t p1, int32_t p2)
{
    uint32_t r = (uint32_t)p0, g = (uint32_t)p1, b = (uint32_t)p2;
    if (model != GF_IMAGE_MODEL_RGB) {
        const uint32_t y = (uint32_t)p0, co = (uint32_t)p1, cg = (uint32_t)p2;
        const uint32_t tmp = y - (uint32_t)gf_img_sar1(cg);
        g = cg + tmp;
        b = tmp - (uint32_t)gf_img_sar1(co);
        r = b + co;
    }
    return (((((0xff00u | r) << 8) | g) << 8) | b);
}

// the reduce window: the channels' sums.  Sums are associative: parts of a window may be accumulated apart and added.
struct GfImgAcc {
    uint32_t r, g, b;
};

GF_HD void gf_img_acc_start(GfImgAcc &a) { a.r = 0, a.g = 0, a.b = 0; }

GF_HD void gf_img_acc_add(GfImgAcc &a, uint32_t w)
{
    a.r += (w >> 16) & 0xffu;
    a.g += (w >> 8) & 0xffu;
    a.b += w & 0xffu;
}

// n = f * f, f in 1 .. GF_IMAGE_MAX_FACTOR: the sums and sum + n / 2 stay below 2^31, so the unsigned division is Java's
GF_HD uint32_t gf_img_acc_finish(const GfImgAcc &a, int32_t n)
{
    const uint32_t un = (uint32_t)n, half = un / 2u;
    const uint32_t r = (a.r + half) / un, g = (a.g + half) / un, b = (a.b + half) / un;
    return 0xff000000u | (r << 16) | (g << 8) | b;
}

// one output word of a reduced image, pixel by pixel: the harness' whole route, and what every kernel path must equal
GF_HD uint32_t gf_img_reduce_word(const uint32_t *argb, int64_t width, int32_t f, int64_t i, int64_t j)
{
    GfImgAcc a;
    gf_img_acc_start(a);
    const uint32_t *p = argb + i * f * width + j * f;
    for (int32_t r = 0; r < f; r++, p += width)
        for (int32_t c = 0; c < f; c++) gf_img_acc_add(a, p[c]);
    return gf_img_acc_finish(a, f * f);
}
