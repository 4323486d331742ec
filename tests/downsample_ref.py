"""A numpy model of the reference's ExampleDownsample loop (demo/src/main/java/org/gridfour/demo/globalDEM/ExampleDownsample.java:
164-210, the grid size of makeSpec :228-239), written from the Java and independent of gridfour_amd/csrc/gvrs_downsample_common.h.

Output cell (i, j) covers source rows i*f .. i*f+f-1 and columns j*f .. j*f+f-1 in row-major order.
  INT, SHORT (:193-206): any cell equal to the fill -> the fill; else int sSum with Java wrap-around (here: exact int64 sums, then a
  mask), avg = (double) sSum / (f*f), (int) Math.floor(avg + 0.5).
  FLOAT (:185-191): float fSum = 0; fSum += f[k] for k in order -- here one float32 addition of whole arrays per k, with a cast
  after every addition -- then fSum / f.length, a float32 division by (float)(f*f).
The rectangle rule for a block that holds the rectangle (row0, col0, n_rows, n_cols) of the source grid: the coarse cells whose
whole window lies inside it, first = ceil(row0 / f), count = floor((row0 + n_rows) / f) - first."""
import numpy as np

INT, SHORT, FLOAT, ICF = 0, 1, 2, 3
DTYPES = {INT: np.int32, SHORT: np.int16, FLOAT: np.float32}


def axis(at, n, f):
    first = -((-at) // f)
    return first, max((at + n) // f - first, 0)


def out_rect(block, f):
    """block = (row0, col0, n_rows, n_cols) on the source grid -> the same on the coarse grid"""
    r0, nr = axis(block[0], block[2], f)
    c0, nc = axis(block[1], block[3], f)
    return (r0, c0, nr, nc)


def windows(values, block, f):
    """[out_rows, out_cols, f*f]: every output cell's window in the reference's order"""
    r0, c0, nr, nc = out_rect(block, f)
    values = np.asarray(values).reshape(block[2], block[3])
    ro, co = r0 * f - block[0], c0 * f - block[1]
    return values[ro:ro + nr * f, co:co + nc * f].reshape(nr, f, nc, f).transpose(0, 2, 1, 3).reshape(nr, nc, f * f)


def downsample_int(values, block, f, fill, dtype=np.int32):
    w = windows(values, block, f).astype(np.int64)
    s = w.sum(axis=2)                                                    # exact: |sum| < 2^31 * f^2
    s = ((s + 2 ** 31) & 0xffffffff) - 2 ** 31                           # Java's int
    avg = s.astype(np.float64) / np.float64(f * f)
    res = np.floor(avg + 0.5).astype(np.int64)
    res[(w == fill).any(axis=2)] = fill
    assert ((res >= np.iinfo(dtype).min) & (res <= np.iinfo(dtype).max)).all()
    return res.astype(dtype)


def downsample_float(values, block, f, row_sums_first=False):
    """row_sums_first: NOT the reference -- each window row summed from 0, the row sums then added in order; what a wrong
    summation order would give, for the tests' own check that their inputs can tell"""
    w = windows(np.asarray(values, np.float32), block, f)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros(w.shape[:2], np.float32)
        if row_sums_first:
            for r in range(f):
                t = np.zeros(w.shape[:2], np.float32)
                for c in range(f):
                    t = (t + w[:, :, r * f + c]).astype(np.float32)
                s = (s + t).astype(np.float32)
        else:
            for k in range(f * f):
                s = (s + w[:, :, k]).astype(np.float32)
        return (s / np.float32(f * f)).astype(np.float32)


def downsample(values, block, f, elem_type, fill=0):
    if elem_type == FLOAT:
        return downsample_float(values, block, f)
    return downsample_int(values, block, f, fill, DTYPES[elem_type])


def same_bits(a, b):
    """bit for bit; a NaN matches any NaN (the reference pins no payload); +0.0 and -0.0 differ"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))
