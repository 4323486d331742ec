"""The values the tests of the writes at scattered points share (test_file_points_write_program.py through the stand-alone program
around the cell rule, test_gpu_file_points_write.py through the library): per element kind every edge of TileElement*.setValue --
the ends of the default range and one step beyond, the fill itself, NaN with a NaN fill and with another, +0.0 / -0.0 against a
0.0 fill, an int-coded float at min_f, max_f, at half-way codes and beyond the range."""
import numpy as np

import block_write_ref as BW

F32 = np.float32
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def f32(x):
    return F32(x)


def bits(a, dtype):
    """the 32 bits a value travels as (a SHORT's: its low 16)"""
    a = np.ascontiguousarray(a, dtype)
    if dtype == np.int16:
        return a.view(np.uint16).astype(np.uint32)
    return a.view(np.uint32)


def icf_values(el):
    lo, hi = BW.default_range(el)
    scale, offset = F32(el[1]), F32(el[2])
    with np.errstate(over="ignore", invalid="ignore"):
        half = [offset + F32(k + 0.5) / scale for k in (0, 1, -1, -2, 100)]       # codes half-way between two integers
        vals = [lo, hi, np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf)), F32(el[4]), F32(np.nan), F32(np.inf), F32(-np.inf),
                F32(0.0), F32(-0.0), offset, F32(1.25), F32(-7.75)] + half
    return np.array(vals, F32)


# (element as GvrsFileHip.elems names it, the fill as the model takes it, the values)
CASES = [
    ("int", INT_MIN, np.array([INT_MIN, INT_MIN + 1, INT_MAX, 0, -1, -9999], np.int32)),
    ("int", -9999, np.array([INT_MIN, INT_MIN + 1, INT_MAX, 0, -1, -9999], np.int32)),
    ("short", -32768, np.array([-32768, -32767, 32767, 0, -1], np.int16)),
    ("short", -1, np.array([-32768, -32767, 32767, 0, -1], np.int16)),
]
_FLOATS = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5, -5.5, 3.4028235e38, 1e-45], F32)
CASES += [("float", fill, _FLOATS) for fill in (float("nan"), 0.0, -5.5)]
for _el in (("icf", 4.0, 8.0, INT_MIN, float("nan")), ("icf", 1.0, 0.0, -1, -9999.0), ("icf", 1000.0, -3.0, INT_MIN, 0.0),
            ("icf", 0.5, 1e6, 7, float("nan"))):
    CASES.append((_el, None, icf_values(_el)))


def expected(el, fill, values):
    """-> (stored [n] bool, the tile's cell as bits [n] (0 where refused), the cell is data [n] bool)"""
    cell, refused = BW.set_values(values, el, fill)
    dt = BW.tile_dtype(el)
    valid = BW.valid_mask(cell, el, fill) & ~refused
    return ~refused, np.where(refused, 0, bits(cell, dt)).astype(np.uint32), valid
