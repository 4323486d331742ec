"""The numpy model of ARGB words stored as element planes and of the reduced image, as the reference computes them: the split
into r, g, b or Y, Co, Cg (demo/imaging/ExperimentalImageStorage.java:203-213, :242-256), the join (:275-286; for r, g, b the same
loop without the transform: the reference has none of its own) and DemoCOG.makeReducedImage (demo/geoTiff/DemoCOG.java:735-770).
Everything is Java's int: int32 arrays whose sums and left shifts are done in int64 and wrapped back explicitly, >> is numpy's
arithmetic shift of a signed value."""
import numpy as np

RGB, YCOCG = 0, 1
MODELS = (RGB, YCOCG)
INT, SHORT = 0, 1                          # GF_ELEM_INT, GF_ELEM_SHORT
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
MAX_FACTOR = 2899


def wrap(x):
    """int64 values -> Java ints"""
    return ((np.asarray(x, np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)


def words(a):
    """ARGB words, given as int32 or as unsigned values, as int32"""
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.uint32 else wrap(a)


def plane_dtype(elem_type):
    return np.int16 if elem_type == SHORT else np.int32


def channels(argb):
    w = words(argb)
    return (w >> 16) & 0xff, (w >> 8) & 0xff, w & 0xff


def split(model, argb):
    """the three planes of argb, int32"""
    r, g, b = channels(argb)
    if model == RGB:
        return [r, g, b]
    co = r - b
    tmp = b + (co >> 1)
    cg = g - tmp
    y = tmp + (cg >> 1)
    return [y, co, cg]


def join(model, planes):
    """the words of any three int arrays (an int16 plane is sign-extended)"""
    p = [np.asarray(x).astype(np.int32) for x in planes]
    if model == RGB:
        r, g, b = p
    else:
        y, co, cg = p
        tmp = wrap(y.astype(np.int64) - (cg >> 1))
        g = wrap(cg.astype(np.int64) + tmp)
        b = wrap(tmp.astype(np.int64) - (co >> 1))
        r = wrap(b.astype(np.int64) + co)
    w = wrap((0xff00 | r).astype(np.int64) << 8) | g
    return wrap(w.astype(np.int64) << 8) | b


def reduce_size(width, height, f):
    return width // f, height // f


def reduce(argb, f):
    """argb [height, width] -> [height // f, width // f] int32"""
    w = words(argb)
    assert w.ndim == 2 and 1 <= f <= MAX_FACTOR
    nr, nc = w.shape[0] // f, w.shape[1] // f
    n = f * f
    out = np.int64(0xff000000)
    for shift in (16, 8, 0):
        c = ((w[:nr * f, :nc * f] >> shift) & 0xff).astype(np.int64).reshape(nr, f, nc, f).sum(axis=(1, 3))
        assert (c + n // 2 <= INT_MAX).all()
        out = out | ((c + n // 2) // n) << shift
    return wrap(out).reshape(nr, nc)
