"""The numpy model of the block tabulation (gf_block_tabulate_*, gf_tab_*), written from the Java text of the reference:
  dense form    demo/.../globalDEM/InputDataStatCollector.java:55-108 (constructor, addSample, getEntropy) beside PackageData's
                zMin / zMax / zSum (PackageData.java:445-448, :504-533) and ExtractData's skipped fill (ExtractData.java:306-317)
  symbol form   demo/.../entropy/EntropyTabulator.java:227-297 (the count per 32-bit symbol, the walk over the count file in
                ascending unsigned order, the Kahan-summed entropy; util/KahanSummation.java:63-69)
The vectorised functions are what the tests compare against; the *_literal functions transcribe the Java loops cell by cell and
hold the vectorised ones to them on small inputs (tests/test_tabulate_ref.py)."""
import math

import numpy as np

INT, SHORT, FLOAT = 0, 1, 2
DTYPES = {INT: np.int32, SHORT: np.int16, FLOAT: np.float32}
SUMMARY_KEYS = ("n_cells", "n_skipped", "n_samples", "sum_samples", "sum_i", "min", "max", "min_at", "max_at")


def _wrap32(x):
    return (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31


def _wrap64(x):
    return (int(x) + 2 ** 63) % 2 ** 64 - 2 ** 63


def java_int(x):
    """Java's (int) of doubles: truncating, saturating, NaN -> 0"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        t = np.clip(np.trunc(x), -2.0 ** 31, 2.0 ** 31 - 1)
    return np.where(np.isnan(x), 0.0, t).astype(np.int64).astype(np.int32)


def plan(def_min, def_max, scale):
    """the constructor: the difference a Java int, the product a double with the scale as given, this.scale a float"""
    scale = float(scale)
    if not scale > 0.0:
        return None
    n_counter = int(java_int(float(_wrap32(def_max - def_min + 1)) * scale))
    if n_counter < 0:
        return None
    with np.errstate(over="ignore"):
        scale_used = float(np.float32(scale))                              # this.scale = (float) scale
    return dict(n_counter=n_counter, base=int(java_int(float(def_min) * scale)), n_bins=n_counter + 1, scale_used=scale_used)


def samples_of(values, scale_used):
    """addSample's `(int) (inputSample * scale + 0.5)`: FP64, one rounding per operation"""
    return java_int(np.asarray(values).astype(np.float64) * np.float64(scale_used) + 0.5)


def empty_summary():
    return dict(n_cells=0, n_skipped=0, n_samples=0, sum_samples=0, sum_i=0, min=math.inf, max=-math.inf, min_at=-1, max_at=-1)


def dense(values, elem_type, def_min, def_max, scale, fill_i=0, skip_fill=False, first_cell=0, into=None, scale_used=None):
    """(counter [n_bins] int32, summary) of one call; into = (counter, summary): accumulate onto them.  scale_used: another scale
    for the samples than the float the constructor keeps (for showing what the float does)"""
    p = plan(def_min, def_max, scale)
    su = p["scale_used"] if scale_used is None else scale_used
    v = np.ascontiguousarray(values, DTYPES[elem_type]).ravel()
    counter = np.zeros(p["n_bins"], np.int64) if into is None else into[0].astype(np.int64)
    s = empty_summary() if into is None else dict(into[1])
    is_sample = ~np.isnan(v) if elem_type == FLOAT else ~((v == fill_i) & bool(skip_fill))
    at = np.flatnonzero(is_sample)
    d = v[at].astype(np.float64)
    sample = samples_of(d, su).astype(np.int64)
    index = (sample - p["base"] + 2 ** 31) % 2 ** 32 - 2 ** 31
    ok = (index >= 0) & (index <= p["n_counter"])
    counter += np.bincount(index[ok], minlength=p["n_bins"])
    s["n_cells"] += v.size
    s["n_skipped"] += v.size - at.size
    s["n_samples"] += int(ok.sum())
    s["sum_samples"] = _wrap64(s["sum_samples"] + int(sample[ok].sum(dtype=np.int64)))
    if elem_type != FLOAT:
        s["sum_i"] = _wrap64(s["sum_i"] + int(v[at].sum(dtype=np.int64)))
    if at.size:
        for key, ext, better in (("min", d.min(), lambda a, b: a < b), ("max", d.max(), lambda a, b: a > b)):
            k = int(np.argmax(d == ext))                                   # the FIRST cell equal to the extreme (+0.0 == -0.0)
            val, where = float(d[k]), first_cell + int(at[k])
            old, old_at = s[key], s[key + "_at"]
            if old_at < 0 or better(val, old) or (val == old and where < old_at):
                s[key], s[key + "_at"] = val, where
    return ((counter + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32), s


def dense_literal(values, elem_type, def_min, def_max, scale, fill_i=0, skip_fill=False, first_cell=0):
    """the Java loops as they stand, one cell at a time (a fresh collector; no accumulate)"""
    def jint(x):
        if x != x:
            return 0
        return int(max(-2.0 ** 31, min(2.0 ** 31 - 1, math.trunc(x)))) if abs(x) != math.inf else (2 ** 31 - 1 if x > 0 else -2 ** 31)
    n_counter = jint(float(_wrap32(def_max - def_min + 1)) * float(scale))
    counter = [0] * (n_counter + 1)
    base = jint(float(def_min) * float(scale))
    scale_f = float(np.float32(scale))                                     # this.scale = (float) scale
    s = empty_summary()
    for i, cell in enumerate(np.ascontiguousarray(values, DTYPES[elem_type]).ravel()):
        s["n_cells"] += 1
        x = float(cell)
        if x != x or (elem_type != FLOAT and skip_fill and int(cell) == fill_i):
            s["n_skipped"] += 1
            continue
        if x < s["min"]:                                                   # PackageData: if (z < zMin) zMin = z
            s["min"], s["min_at"] = x, first_cell + i
        if x > s["max"]:
            s["max"], s["max_at"] = x, first_cell + i
        if elem_type != FLOAT:
            s["sum_i"] = _wrap64(s["sum_i"] + int(cell))
        sample = jint(x * scale_f + 0.5)
        index = _wrap32(sample - base)
        if index < 0 or index > n_counter:
            continue
        counter[index] = _wrap32(counter[index] + 1)
        s["sum_samples"] = _wrap64(s["sum_samples"] + sample)
        s["n_samples"] += 1
    return np.array(counter, np.int32), s


def keys_of(values, elem_type):
    """EntropyTabulator's symbol per cell: readValueInt's int (a short sign-extended) or floatToRawIntBits, as unsigned"""
    v = np.ascontiguousarray(values, DTYPES[elem_type]).ravel()
    return v.astype(np.int32).view(np.uint32) if elem_type == SHORT else v.view(np.uint32)


def symbols(values, elem_type):
    """(symbols uint32 ascending unsigned, counts int32, summary) -- the table is not cut to any capacity"""
    sym, cnt = np.unique(keys_of(values, elem_type), return_counts=True)
    s = dict(n_samples=int(cnt.sum()), n_symbols=int(sym.size), n_unique=int((cnt == 1).sum()), n_repeated=int((cnt != 1).sum()),
             n_written=int(sym.size), max_count=int(cnt.max()) if cnt.size else 0, reserved=0)
    return sym.astype(np.uint32), cnt.astype(np.int32), s


def symbols_literal(values, elem_type):
    """the survey loop and the walk over the count file, one cell and one counter at a time"""
    counts = {}
    n_samples = n_symbols = 0
    for bits in keys_of(values, elem_type).tolist():
        long_index = bits & 0xffffffff
        count = counts.get(long_index, 0)
        counts[long_index] = count + 1
        n_samples += 1
        if count == 0:
            n_symbols += 1
    max_count = n_unique = n_repeated = 0
    sym, cnt = [], []
    for key in sorted(counts):                                             # rows, then columns, of the count file
        count = counts[key]
        if count > 0:
            sym.append(key)
            cnt.append(count)
            max_count = max(max_count, count)
            if count == 1:
                n_unique += 1
            else:
                n_repeated += 1
    s = dict(n_samples=n_samples, n_symbols=n_symbols, n_unique=n_unique, n_repeated=n_repeated, n_written=n_symbols, max_count=max_count,
             reserved=0)
    return np.array(sym, np.uint32), np.array(cnt, np.int32), s


def entropy(counts, n_samples, kahan):
    """bits per sample from counts in the order given.  kahan: EntropyTabulator.java:265-297 with KahanSummation.add as written;
    else InputDataStatCollector.getEntropy.  math.log is the C library's log, as the library's is."""
    if not kahan and n_samples == 0:
        return 0.0
    d = float(n_samples)
    if kahan:
        c = s = 0.0
        for count in np.asarray(counts).tolist():
            if count > 0:
                p = float(count) / d
                a = -p * math.log(p)
                y = a - c
                t = s + y
                c = (t - s) - y
                s = t
        return s / math.log(2.0)
    total = 0.0
    for count in np.asarray(counts).tolist():
        if count > 0:
            p = float(count) / d
            total += p * math.log(p)
    return -total / math.log(2.0)


def bits(x):
    return np.float64(x).view(np.uint64).item()


def same_summary(got, want):
    """every field equal, min / max bit for bit"""
    return all((bits(got[k]) == bits(want[k])) if k in ("min", "max") else (int(got[k]) == int(want[k])) for k in want)
