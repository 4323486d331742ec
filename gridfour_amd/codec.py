"""Host-side mirror of the reference plug-in interface for the HIP codec.

`CodecHuffmanHip` carries the method names, argument meaning and error behaviour of the
reference's `ICompressionEncoder` / `ICompressionDecoder` as implemented by `CodecHuffman`
(core/src/main/java/org/gridfour/compress/ICompressionEncoder.java:61-91,
ICompressionDecoder.java:62-105, CodecHuffman.java:70-153):

  encode(codecIndex, nRows, nCols, values) -> bytes | None      (None = Java null)
  decode(nRows, nColumns, packing) -> int32 array, raises IOError (= IOException)
  encodeFloats / decodeFloats -> None, implementsIntegerEncoding() -> True, ...

plus the batched forms the GPU needs (one launch per batch of tiles, not per tile).
All compute happens in libgvrs_hip.so; nothing here has a CPU implementation.

The module in order: constants and struct dtypes; helpers, DeviceBuffer and the device-call scope; GvrsHipContext and the objects
made on one; the codec classes.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib

# ---- constants and struct dtypes (include/gvrs_hip_codec.h) ----
INT4_NULL_CODE = -(2 ** 31)   # util/GridfourConstants.java:61

CODEC_NONE, CODEC_HUFFMAN, CODEC_DEFLATE, CODEC_CANON_HUFFMAN, CODEC_LSOP12, CODEC_LSOP08 = 0, 1, 2, 3, 4, 5
CODEC_UNKNOWN = -1             # GF_CODEC_UNKNOWN: a file's codec id the library has no decoder for
STANDARD_CODEC_LIST = (CODEC_HUFFMAN, CODEC_DEFLATE, CODEC_NONE, CODEC_CANON_HUFFMAN)    # GvrsFileSpecification.java:221-230

# What an element kind means, in one place.  type: its GF_ELEM_* number; delivered: the dtype a reader hands out; written: the dtype
# a record writer takes (an int-coded float's int32 codes); coarse: the dtype of a downsampled block; fill: the gf_elem_spec field
# of a block's fill cell and its default (None: an int-coded float's is the fill_f of its description); range: the gf_elem_range
# fields' suffix and the default range (an int-coded float's in codes, which its scale and offset turn into values).
_ElemKind = collections.namedtuple("_ElemKind", "type delivered written coarse fill range")
_ELEM_KINDS = {
    "int": _ElemKind(0, np.int32, np.int32, np.int32, ("fill_i", INT4_NULL_CODE), ("i", INT4_NULL_CODE + 1, 2 ** 31 - 1)),
    "short": _ElemKind(1, np.int16, np.int16, np.int16, ("fill_i", -32768), ("i", -32767, 32767)),
    "float": _ElemKind(2, np.float32, np.float32, np.float32, ("fill_f", np.float32(np.nan)), ("f", -np.inf, np.inf)),
    "icf": _ElemKind(3, np.float32, np.int32, np.int32, None, ("f", INT4_NULL_CODE + 1, 2 ** 31 - 2)),
}
ELEM_TYPES = {name: kind.type for name, kind in _ELEM_KINDS.items()}                       # GF_ELEM_*
_DELIVERED = {kind.type: kind.delivered for kind in _ELEM_KINDS.values()}
_ELEM_SPEC = np.dtype([("type", np.int32), ("fill_i", np.int32), ("scale", np.float32), ("offset", np.float32),
                       ("fill_f", np.float32)])                                           # gf_elem_spec
_ELEM_RANGE = np.dtype([("min_i", np.int32), ("max_i", np.int32), ("min_f", np.float32), ("max_f", np.float32)])   # gf_elem_range
_FILE_INFO = np.dtype([("version", np.int32), ("subversion", np.int32), ("checksum_enabled", np.int32), ("raster_space", np.int32),
                       ("coordinate_system", np.int32), ("grid", np.int32, 4), ("n_elems", np.int32), ("elems", _ELEM_SPEC, 16),
                       ("n_codecs", np.int32), ("codecs", np.int32, 255), ("content_pos", np.uint64), ("tile_dir_pos", np.uint64),
                       ("metadata_dir_pos", np.uint64), ("freespace_dir_pos", np.uint64), ("dir_extended", np.int32), ("dir_row0", np.int32),
                       ("dir_col0", np.int32), ("dir_n_rows", np.int32), ("dir_n_cols", np.int32), ("dir_entries_pos", np.uint64),
                       ("x0", np.float64), ("y0", np.float64), ("x1", np.float64), ("y1", np.float64), ("cell_size_x", np.float64),
                       ("cell_size_y", np.float64), ("m2r", np.float64, 6), ("r2m", np.float64, 6)], align=True)         # gf_file_info
_FILE_RECORD = np.dtype([("pos", np.uint64), ("size", np.uint32), ("type", np.int32), ("tile_index", np.int32), ("checksum", np.int32)],
                        align=True)                                                       # gf_file_record
_FILE_INSPECT_REPORT = np.dtype([("status", np.int32), ("failed", np.int32), ("complete", np.int32), ("stop", np.int32),
                                 ("bad_tile_index", np.int32), ("invalid_record_size", np.int32), ("tile_dir_located", np.int32),
                                 ("tile_dir_passed", np.int32), ("termination_pos", np.uint64), ("n_records", np.uint64),
                                 ("n_by_type", np.uint64, 7), ("n_checksum_failures", np.uint64), ("n_bad_tiles", np.uint64)],
                                align=True)                                               # gf_file_inspect_report
INSPECT_STOPS = ("end", "bad_tile_index", "tile_too_large", "two_checksum_failures", "bad_record_type", "bad_record_size", "truncated")

_FILE_ELEM_FACTS = np.dtype([("name", np.uint64), ("label", np.uint64), ("description", np.uint64), ("unit", np.uint64), ("continuous", np.int32),
                             ("has_range", np.int32), ("range", _ELEM_RANGE)], align=True)                             # gf_file_elem_facts
_FILE_FACTS = np.dtype([("grid", np.int32, 4), ("n_elems", np.int32), ("n_codecs", np.int32), ("elems", np.uint64), ("elem_facts", np.uint64),
                        ("codec_ids", np.uint64), ("product_label", np.uint64), ("checksum_enabled", np.int32), ("raster_space", np.int32),
                        ("coordinate_system", np.int32), ("reserved", np.int32), ("x0", np.float64), ("y0", np.float64), ("x1", np.float64),
                        ("y1", np.float64), ("cell_size_x", np.float64), ("cell_size_y", np.float64), ("m2r", np.float64, 6),
                        ("r2m", np.float64, 6), ("uuid", np.uint8, 16), ("time_modified", np.int64)], align=True)           # gf_file_facts
_FILE_METADATA = np.dtype([("name", np.uint64), ("description", np.uint64), ("content", np.uint64), ("content_bytes", np.uint64),
                           ("record_id", np.int32), ("type", np.int32)], align=True)                                     # gf_file_metadata
FILE_DIR_EXTENDED = 1                                                      # GF_FILE_DIR_EXTENDED

IMAGE_RGB, IMAGE_YCOCG = 0, 1                                              # GF_IMAGE_*
IMAGE_MODELS = {"rgb": IMAGE_RGB, "ycocg": IMAGE_YCOCG}
TAB_ACCUMULATE, TAB_SKIP_FILL = 1, 2                                      # GF_TAB_*
TAB_SYM_INPUT_TRUNCATED = 1                                               # GF_TAB_SYM_INPUT_TRUNCATED
_TAB_DENSE = np.dtype([("def_min", np.int32), ("def_max", np.int32), ("scale", np.float64)])                          # gf_tab_dense
_TAB_DENSE_PLAN = np.dtype([("n_counter", np.int32), ("base", np.int32), ("n_bins", np.int64), ("scale_used", np.float64)])   # gf_tab_dense_plan
TAB_SUMMARY = np.dtype([("n_cells", np.int64), ("n_skipped", np.int64), ("n_samples", np.int64), ("sum_samples", np.int64), ("sum_i", np.int64),
                        ("min", np.float64), ("max", np.float64), ("min_at", np.int64), ("max_at", np.int64)])       # gf_tab_summary
TAB_SYMBOLS = np.dtype([("n_samples", np.int64), ("n_symbols", np.int64), ("n_unique", np.int64), ("n_repeated", np.int64),
                        ("n_written", np.int64), ("max_count", np.int32), ("reserved", np.int32)])                   # gf_tab_symbols

INTERP_VALUE, INTERP_FIRST, INTERP_SECOND = 0, 1, 2                      # GF_INTERP_*
_INTERP_SPEC = np.dtype([("n_rows_grid", np.int32), ("n_cols_grid", np.int32), ("block", np.int32, 4), ("elem_type", np.int32),
                         ("fill_i", np.int32), ("wrap", np.int32), ("target", np.int32), ("row_spacing", np.float64),
                         ("col_spacing", np.float64), ("row_fringe0", np.float64), ("row_fringe1", np.float64),
                         ("col_fringe0", np.float64), ("col_fringe1", np.float64)], align=True)                      # gf_interp_spec
COORDS_GRID, COORDS_FILE = 0, 1                                          # GF_COORDS_*
MAP_GEO_TO_GRID, MAP_MODEL_TO_GRID, MAP_GRID_TO_GEO, MAP_GRID_TO_MODEL = 0, 1, 2, 3   # GF_MAP_*
_INTERP_OUT = np.dtype([(k, np.uint64) for k in ("z", "zx", "zy", "zxx", "zxy", "zyy", "normal", "status")])        # gf_interp_out
_INTERP_LATTICE = np.dtype([("row0", np.float64), ("col0", np.float64), ("row_step", np.float64), ("col_step", np.float64),
                            ("n_rows", np.int64), ("n_cols", np.int64)])                                            # gf_interp_lattice

PALETTE_RGB, PALETTE_HSV, PALETTE_MAX_RECORDS, RENDER_UNLIMITED, RENDER_Z = 0, 1, 256, 1, 4                                     # GF_PALETTE_*, GF_RENDER_*
_PALETTE_RECORD = np.dtype([("range0", np.float64), ("range1", np.float64), ("model", np.int32), ("rgb0", np.int32, 3), ("rgb1", np.int32, 3),
                            ("reserved", np.int32), ("hsv0", np.float64, 3), ("hsv1", np.float64, 3)])               # gf_palette_record
_PALETTE_SPEC = np.dtype([("records", np.uint64), ("n_records", np.int32), ("argb_for_null", np.uint32), ("normalized", np.int32),
                          ("hinge", np.int32), ("range_min", np.float64), ("range_max", np.float64), ("hinge_value", np.float64)])  # gf_palette_spec
_RENDER_LIGHT = np.dtype([("x_gain", np.float64), ("y_gain", np.float64), ("sun", np.float64, 3), ("ambient", np.float64)])  # gf_render_light
_RENDER_OUT = np.dtype([(k, np.uint64) for k in ("argb", "shade", "status")])                                       # gf_render_out

# struct gf_codec_stats (include/gvrs_hip_codec.h) = the sums of compress/CodecStats.java
CODEC_STATS_DTYPE = np.dtype([("n_tiles", "<i8"), ("n_bytes", "<i8"), ("n_symbols", "<i8"), ("n_bits_overhead", "<i8"),
                              ("n_m32_counted", "<i8"), ("sum_length_m32", "<i8"), ("sum_observed_m32", "<i8"),
                              ("sum_entropy_m32", "<f8")])

# struct gf_canon_stats (include/gvrs_hip_codec.h) = the sums of compress/canonicalHuffman/CanonHuffmanStats.java
CANON_STATS_DTYPE = np.dtype([("n_tiles", "<i8"), ("n_bytes", "<i8"), ("n_symbols", "<i8"), ("n_bits_overhead", "<i8"),
                              ("n_text_counted", "<i8"), ("sum_length", "<i8"), ("sum_observed", "<i8"), ("sum_entropy", "<f8"),
                              ("sum_escape_bits", "<i8")])


# ---- helpers ----
def _call(name, *args):
    """The entry point `name` of the library called and its status checked: raises GvrsHipError, else returns the status."""
    return check(getattr(lib(), name)(*args), name)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _ptrs(items):
    """The c_void_p array of a per-element pointer table: items are DeviceBuffers, host arrays, c_void_p or plain addresses."""
    def address(p):
        if isinstance(p, DeviceBuffer):
            return p.ptr.value
        if isinstance(p, np.ndarray):
            return p.ctypes.data
        return p.value if isinstance(p, C.c_void_p) else p
    return (C.c_void_p * len(items))(*[address(p) for p in items])


def _blob_of(packings):
    """(blob, offsets[n + 1]) of packings laid back to back, with 16 zero bytes behind the last: the kernels read whole aligned
    words past a packing's end."""
    offsets = np.zeros(len(packings) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(p) for p in packings])
    return np.frombuffer(b"".join(packings) + b"\0" * 16, dtype=np.uint8), offsets


def _records_in(blob, offsets, tail=False):
    """Records as a caller hands them in -> (blob uint8, offsets uint64), both contiguous; tail: with the 16 zero bytes behind the
    blob that a host form reads into."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    if tail:
        blob = np.concatenate([blob, np.zeros(16, np.uint8)])
    return blob, np.ascontiguousarray(offsets, dtype=np.uint64)


def _records_out(blob, offsets, n, status=None):
    """The n records blob[offsets[t]:offsets[t + 1]] as a list of bytes; with status, None for a record whose status is not OK."""
    return [bytes(blob[int(offsets[t]):int(offsets[t + 1])]) if status is None or status[t] == _lib.OK else None for t in range(n)]


def _old_records(old):
    """The old= argument of the writers, None or (blob, offsets) -> (blob, offsets, number of records); None: 16 bytes, no record."""
    if old is None:
        return np.zeros(16, np.uint8), np.zeros(1, np.uint64), 0
    old_blob, old_off = _records_in(*old)
    return old_blob, old_off, old_off.size - 1


def _grown_blob(encode, cap, slack, offsets):
    """The blob of a host-form batch encoder that answers ERR_CAPACITY with the bytes it needs in offsets[-1]: encode(blob, cap)
    is called until the blob holds them.  Returns (the last call's status, unchecked; blob)."""
    while True:
        blob = np.empty(max(cap, 16), np.uint8)
        st = encode(blob, cap)
        if st != _lib.ERR_CAPACITY:
            return st, blob
        cap = int(offsets[-1]) + slack


def _grid_rect(nRows, nCols, grid_shape, rect):
    """(grid, rect) as the block entry points take them: (rows, columns of the grid, rows, columns of a tile), (row0, col0, n_rows, n_cols)"""
    return np.array([grid_shape[0], grid_shape[1], nRows, nCols], np.int32), np.ascontiguousarray(rect, np.int32)


def _tiles_of_rect(grid, rect):
    """gf_block_tile_rect: how many tiles rect touches"""
    tr = tuple(C.c_int32() for _ in range(4))
    _call("gf_block_tile_rect", _ptr(grid), _ptr(rect), *[C.byref(x) for x in tr])
    return tr[2].value * tr[3].value


def _argb_words(argb):
    """ARGB words as int32: uint32 words keep their bits, anything else is converted"""
    a = np.asarray(argb)
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a, np.int32)


def _out_struct(dtype, out):
    """A struct of output addresses (gf_interp_out, gf_render_out) from a dict of c_void_p, addresses or None under its field names"""
    o = np.zeros(1, dtype)
    for k, v in out.items():
        o[k] = 0 if v is None else (v.value if isinstance(v, C.c_void_p) else int(v)) or 0
    return o


def _lattice_struct(lattice):
    """A gf_interp_lattice from (row0, col0, row_step, col_step, n_rows, n_cols)"""
    lat = np.zeros(1, _INTERP_LATTICE)
    lat["row0"], lat["col0"], lat["row_step"], lat["col_step"], lat["n_rows"], lat["n_cols"] = lattice
    return lat


def _elem_kind(el):
    """An elems entry "int" | "short" | "float" | ("icf", scale, offset, fill_i, fill_f) -> (kind, its _ELEM_KINDS row, the
    entry's parameters (scale, offset, fill_i, fill_f) or None)"""
    kind = el if isinstance(el, str) else el[0]
    return kind, _ELEM_KINDS[kind], (None if kind != "icf" else tuple(el[1:]))


def _elem_type(x):
    """GF_ELEM_* of an element's name or number"""
    return ELEM_TYPES[x] if isinstance(x, str) else int(x)


def _delivered_dtype(elem_type):
    """The dtype of a GF_ELEM_* number's delivered cells; float32 for a number that is none (the library refuses it)"""
    return _DELIVERED.get(int(elem_type), np.float32)


def _tab_dense_spec(def_min, def_max, scale):
    s = np.zeros(1, _TAB_DENSE)
    s["def_min"], s["def_max"], s["scale"] = def_min, def_max, scale
    return s


def _tab_table_in(table):
    """A symbol table as the host forms take it in: None (empty) or (symbols, counts, summary dict) -> (symbols uint32, counts
    int32, gf_tab_symbols [1] or None, the arguments: three pointers and the cap)"""
    if table is None:
        return None, None, None, (None, None, None, 0)
    sym, cnt = np.ascontiguousarray(table[0], np.uint32).ravel(), np.ascontiguousarray(table[1], np.int32).ravel()
    assert sym.size == cnt.size
    summary = np.zeros(1, TAB_SYMBOLS)
    for k in TAB_SYMBOLS.names:
        summary[k] = table[2][k]
    return sym, cnt, summary, (_ptr(sym) if sym.size else None, _ptr(cnt) if sym.size else None, _ptr(summary), sym.size)


def _tab_table_out(name, cap, call):
    """The out table of a host form: call(symbols pointer, counts pointer, cap, summary pointer) -> status; a table that does not
    hold every symbol (ERR_CAPACITY) comes back with what it has -> (symbols, counts, summary dict)"""
    symbols, counts, summary = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.int32), np.zeros(1, TAB_SYMBOLS)
    st = call(_ptr(symbols) if cap else None, _ptr(counts) if cap else None, cap, _ptr(summary))
    if st != _lib.ERR_CAPACITY:
        check(st, name)
    n = int(summary["n_written"][0])
    return symbols[:n], counts[:n], {k: summary[k][0].item() for k in TAB_SYMBOLS.names}


def interp_spec(n_rows_grid, n_cols_grid, block=None, elem_type="float", fill_i=0, wrap=0, target=INTERP_VALUE, row_spacing=1.0,
                col_spacing=1.0, row_fringe=None, col_fringe=None):
    """A gf_interp_spec: the raster's size, the rectangle block = (row0, col0, n_rows, n_cols) of it that the block holds (None:
    all of it), the element ("int", "short", "float", "icf" or GF_ELEM_*; fill_i: the cell of an int / short element that reads as
    NaN), wrap (0; 1 the longitudes wrap; 2 they wrap and bracket), the target and the spacings dv, du of the derivatives.
    The default fringe is (-0.5, n - 0.5) per axis: the reference widens it by 4 ulp of the grid's size, (double) n, on either
    side (GvrsFileSpecification.java:435-440) -- GvrsFileHip.coords_spec() gives those fringes, with wrap and the spacings, for
    a file; a caller that works without a file passes the fringes."""
    s = np.zeros(1, _INTERP_SPEC)
    s["n_rows_grid"], s["n_cols_grid"] = n_rows_grid, n_cols_grid
    s["block"] = (0, 0, n_rows_grid, n_cols_grid) if block is None else block
    s["elem_type"] = _elem_type(elem_type)
    s["fill_i"], s["wrap"], s["target"], s["row_spacing"], s["col_spacing"] = fill_i, wrap, target, row_spacing, col_spacing
    s["row_fringe0"], s["row_fringe1"] = (-0.5, n_rows_grid - 0.5) if row_fringe is None else row_fringe
    s["col_fringe0"], s["col_fringe1"] = (-0.5, n_cols_grid - 0.5) if col_fringe is None else col_fringe
    return s


def palette_records(records):
    """A gf_palette_record array from tuples (range0, range1, "rgb", (r, g, b), (r, g, b)) or (range0, range1, "hsv", (h, s, v),
    (h, s, v)); an array of that dtype passes through."""
    if isinstance(records, np.ndarray) and records.dtype == _PALETTE_RECORD:
        return np.ascontiguousarray(records)
    out = np.zeros(len(records), _PALETTE_RECORD)
    for o, (range0, range1, model, c0, c1) in zip(out, records):
        o["range0"], o["range1"] = range0, range1
        if model in ("rgb", PALETTE_RGB):
            o["model"], o["rgb0"], o["rgb1"] = PALETTE_RGB, c0, c1
        else:
            o["model"], o["hsv0"], o["hsv1"] = (PALETTE_HSV if model == "hsv" else model), c0, c1
    return out


def palette_spec(records, argb_for_null=0, normalized=False, range_min=0.0, range_max=0.0, hinge=False, hinge_value=0.0):
    """(gf_palette_spec, the record array it points to)"""
    recs = palette_records(records)
    s = np.zeros(1, _PALETTE_SPEC)
    s["records"], s["n_records"], s["argb_for_null"] = recs.ctypes.data, len(recs), int(argb_for_null) & 0xffffffff
    s["normalized"], s["hinge"], s["range_min"], s["range_max"], s["hinge_value"] = bool(normalized), bool(hinge), range_min, range_max, hinge_value
    return s, recs


def render_light(x_gain, y_gain, sun, ambient):
    """A gf_render_light: the gains on zx and zy (ExtractData: -steepen, +steepen; DemoCOG: both -steepen), the unit vector
    towards the sun and the ambient level."""
    li = np.zeros(1, _RENDER_LIGHT)
    li["x_gain"], li["y_gain"], li["sun"], li["ambient"] = x_gain, y_gain, sun, ambient
    return li


# ---- device memory: one allocation, and the allocations of one call ----
class DeviceBuffer:
    """A raw device allocation owned through the C ABI (no torch needed)."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _call("gf_dev_malloc", ctx.handle, max(self.nbytes, 16), C.byref(p))
        self.ptr = p

    def upload(self, array, byte_offset=0):
        a = np.ascontiguousarray(array)
        assert byte_offset + a.nbytes <= max(self.nbytes, 16)
        _call("gf_dev_upload", self.ctx.handle, C.c_void_p(self.ptr.value + byte_offset), _ptr(a), a.nbytes)
        return self

    def download(self, dtype, count, byte_offset=0):
        out = np.empty(count, dtype)
        assert byte_offset + out.nbytes <= max(self.nbytes, 16)
        _call("gf_dev_download", self.ctx.handle, _ptr(out), C.c_void_p(self.ptr.value + byte_offset), out.nbytes)
        return out

    def fill(self, value=0):
        _call("gf_dev_memset", self.ctx.handle, self.ptr, value, self.nbytes)
        return self

    def free(self):
        if self.ptr:
            lib().gf_dev_free(self.ctx.handle, self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _DeviceScope:
    """The device buffers of one call: `with _DeviceScope(ctx) as s:` owns every buffer made through s and frees them all when
    the block ends, however it ends -- an allocation or an upload that raised half way included."""

    def __init__(self, ctx):
        self.ctx, self._buffers = ctx, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self._buffers:
            b.free()
        return False

    def alloc(self, nbytes, fill=None):
        """A buffer of nbytes; fill: the byte it is set to"""
        b = DeviceBuffer(self.ctx, nbytes)
        self._buffers.append(b)
        return b if fill is None else b.fill(fill)

    def upload(self, array, slack=0, fill=None):
        """A buffer that holds array and slack bytes behind it (fill: set to that byte first)"""
        a = np.ascontiguousarray(array)
        return self.alloc(a.nbytes + slack, fill).upload(a)

    ptrs = staticmethod(_ptrs)

    def run(self, name, *args):
        """_call, then the context synchronised: after it the buffers may be downloaded"""
        st = _call(name, *args)
        self.ctx.synchronize()
        return st


# ---- the context and the objects made on one ----
class GvrsHipContext:
    """One device context (stream + workspace); one per process and GPU."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _call("gf_context_create", int(device), C.byref(self._h))
        self.device = int(device)

    @property
    def handle(self):
        return self._h

    @property
    def stream(self):
        return lib().gf_context_stream(self._h)

    def synchronize(self):
        _call("gf_context_synchronize", self._h)

    def reserve(self, n_rows, n_cols, n_tiles):
        _call("gf_context_reserve", self._h, n_rows, n_cols, n_tiles)

    def block_from_tiles_dev(self, grid, rect, elem_type, fill_bits, n_tiles, d_tile_indices, d_tiles, d_block, d_tile_status=None,
                             stream=None):
        """gf_block_from_tiles_dev on device pointers: grid = (n_rows_grid, n_cols_grid, n_rows_tile, n_cols_tile), rect = (row0,
        col0, n_rows, n_cols), elem_type one of ELEM_TYPES' values.  Enqueues only."""
        grid, rect = np.ascontiguousarray(grid, np.int32), np.ascontiguousarray(rect, np.int32)
        assert grid.size == 4 and rect.size == 4
        _call("gf_block_from_tiles_dev", self._h, stream, _ptr(grid), _ptr(rect), int(elem_type), int(fill_bits) & 0xffffffff, int(n_tiles),
              d_tile_indices, d_tile_status, d_tiles, d_block)

    def tiles_from_block_dev(self, grid, rect, elem_type, fill_bits, d_block, n_tiles, d_tile_indices, d_tiles, d_status=None,
                             keep_outside=False, stream=None):
        """gf_tiles_from_block_dev on device pointers, the inverse of block_from_tiles_dev.  Enqueues only."""
        grid, rect = np.ascontiguousarray(grid, np.int32), np.ascontiguousarray(rect, np.int32)
        assert grid.size == 4 and rect.size == 4
        _call("gf_tiles_from_block_dev", self._h, stream, _ptr(grid), _ptr(rect), int(elem_type), int(fill_bits) & 0xffffffff,
              int(bool(keep_outside)), d_block, int(n_tiles), d_tile_indices, d_tiles, d_status)

    # ---- a grid block interpolated: B-spline value, derivatives, unit normal (gf_block_interp_*) ----
    @staticmethod
    def _interp_out(out):
        return _out_struct(_INTERP_OUT, out)

    def interp_points_dev(self, spec, d_block, n_points, d_rows, d_cols, out, d_col_spacing=None, stream=None):
        """gf_block_interp_points_dev on device pointers: spec from interp_spec(), out a dict of device pointers under the names
        z, zx, zy, zxx, zxy, zyy, normal (3 doubles per point), status (int32); all but z may be missing.  Enqueues only."""
        o = self._interp_out(out)
        _call("gf_block_interp_points_dev", self._h, stream, _ptr(spec), d_block, int(n_points), d_rows, d_cols, d_col_spacing, _ptr(o))

    def interp_lattice_dev(self, spec, d_block, lattice, out, d_col_spacing_rows=None, stream=None):
        """gf_block_interp_lattice_dev: lattice = (row0, col0, row_step, col_step, n_rows, n_cols); point (i, j) is row0 + i *
        row_step, col0 + j * col_step; outputs row-major n_rows x n_cols; d_col_spacing_rows: one spacing per lattice row.
        Enqueues only."""
        lat, o = _lattice_struct(lattice), self._interp_out(out)
        _call("gf_block_interp_lattice_dev", self._h, stream, _ptr(spec), d_block, _ptr(lat), d_col_spacing_rows, _ptr(o))

    def interp_points(self, spec, block, rows, cols, col_spacing=None):
        """gf_block_interp_points, the host-memory form (staged by the library): block is the rectangle spec["block"] of the raster
        in the element's delivered dtype, rows / cols grid coordinates.  Returns a dict: z and status [n] always; zx, zy and normal
        [n, 3] with target >= INTERP_FIRST; zxx, zxy, zyy with INTERP_SECOND.  A point whose status is not 0 is NaN throughout."""
        rows, cols = np.ascontiguousarray(rows, np.float64).ravel(), np.ascontiguousarray(cols, np.float64).ravel()
        assert rows.size == cols.size
        n, target = rows.size, int(spec["target"][0])
        block = np.ascontiguousarray(block, _delivered_dtype(spec["elem_type"][0]))
        assert block.size == int(spec["block"][0][2]) * int(spec["block"][0][3])
        names = ["z"] + (["zx", "zy"] if target >= INTERP_FIRST else []) + (["zxx", "zxy", "zyy"] if target >= INTERP_SECOND else [])
        res = {k: np.zeros(n, np.float64) for k in names}
        if target >= INTERP_FIRST:
            res["normal"] = np.zeros((n, 3), np.float64)
        res["status"] = np.zeros(n, np.int32)
        cs = None if col_spacing is None else np.ascontiguousarray(col_spacing, np.float64).ravel()
        assert cs is None or cs.size == n
        o = self._interp_out({k: a.ctypes.data for k, a in res.items()})
        _call("gf_block_interp_points", self._h, _ptr(spec), _ptr(block), n, _ptr(rows), _ptr(cols), None if cs is None else _ptr(cs), _ptr(o))
        return res

    # ---- a grid block rendered to ARGB: colour palette and shaded relief (gf_block_render_*) ----
    @staticmethod
    def _render_args(lattice, light, out):
        lat = None if lattice is None else _lattice_struct(lattice)
        return lat, (None if light is None else np.ascontiguousarray(light, _RENDER_LIGHT).reshape(1)), _out_struct(_RENDER_OUT, out)

    def render_cells_dev(self, palette, elem_type, d_cells, n_cells, d_argb, d_shade=None, fill_i=0, unlimited=False, stream=None):
        """gf_block_render_cells_dev on device pointers: n_cells cells of the element ("int", "short", "float", "icf", GF_ELEM_*, or
        "z" / RENDER_Z: doubles) -> d_argb [n_cells] int32; d_shade: one double per cell (the WithShade lookups).  Enqueues only."""
        et = RENDER_Z if elem_type == "z" else _elem_type(elem_type)
        _call("gf_block_render_cells_dev", self._h, stream, palette.handle, RENDER_UNLIMITED if unlimited else 0, et, int(fill_i), d_cells,
              int(n_cells), d_shade, d_argb)

    def render_lattice_dev(self, spec, d_block, lattice, palette, out, light=None, unlimited=False, stream=None):
        """gf_block_render_lattice_dev: spec and lattice as interp_lattice_dev takes them, light from render_light() (None: the
        value alone, no shade), out a dict of device pointers under the names argb (int32), shade (double), status (int32), each
        one item per pixel; argb or shade must be there.  Enqueues only."""
        lat, li, o = self._render_args(lattice, light, out)
        _call("gf_block_render_lattice_dev", self._h, stream, _ptr(spec), d_block, _ptr(lat), palette.handle, None if li is None else _ptr(li),
              RENDER_UNLIMITED if unlimited else 0, _ptr(o))

    def render_points_dev(self, spec, d_block, palette, out, lattice=None, n_points=0, d_rows=None, d_cols=None, d_col_spacing=None,
                          light=None, unlimited=False, stream=None):
        """gf_block_render_points_dev: with lattice, a lattice whose column spacing differs per row (d_col_spacing: one per lattice
        row); without, n_points points d_rows, d_cols (d_col_spacing: one per point).  Enqueues only."""
        lat, li, o = self._render_args(lattice, light, out)
        _call("gf_block_render_points_dev", self._h, stream, _ptr(spec), d_block, None if lat is None else _ptr(lat), int(n_points), d_rows,
              d_cols, d_col_spacing, palette.handle, None if li is None else _ptr(li), RENDER_UNLIMITED if unlimited else 0, _ptr(o))

    def render_lattice(self, spec, block, lattice, palette, light=None, unlimited=False):
        """gf_block_render_lattice, the host-memory form (staged by the library): returns a dict argb [n_rows, n_cols] int32, status
        the same, and shade (float64) with a light."""
        block = np.ascontiguousarray(block, _delivered_dtype(spec["elem_type"][0]))
        assert block.size == int(spec["block"][0][2]) * int(spec["block"][0][3])
        shape = (int(lattice[4]), int(lattice[5]))
        res = {"argb": np.zeros(shape, np.int32), "status": np.zeros(shape, np.int32)}
        if light is not None:
            res["shade"] = np.zeros(shape, np.float64)
        lat, li, o = self._render_args(lattice, light, {k: a.ctypes.data for k, a in res.items()})
        _call("gf_block_render_lattice", self._h, _ptr(spec), _ptr(block), _ptr(lat), palette.handle, None if li is None else _ptr(li),
              RENDER_UNLIMITED if unlimited else 0, _ptr(o))
        return res

    # ---- a grid block downsampled: the box average by an integer factor (gf_block_downsample_*) ----
    @staticmethod
    def downsample_rect(block, factor):
        """gf_block_downsample_rect: block = (row0, col0, n_rows, n_cols) on the source grid -> the rectangle of the coarse grid
        whose cells' whole factor x factor windows lie inside block (n_rows or n_cols may be 0)."""
        block, out = np.ascontiguousarray(block, np.int32), np.zeros(4, np.int32)
        assert block.size == 4
        _call("gf_block_downsample_rect", _ptr(block), int(factor), _ptr(out))
        return tuple(int(x) for x in out)

    @staticmethod
    def _downsample_specs(elems, fills):
        """elems: a gf_elem_spec array as it is, or per element "int" | "short" | "float" with fills as read_block_dev takes them"""
        if isinstance(elems, np.ndarray):
            assert elems.dtype == _ELEM_SPEC and fills is None
            return elems, [_delivered_dtype(t) for t in elems["type"]]
        specs, dtypes = CodecMasterHip._elem_specs(elems)
        return CodecMasterHip._fill_specs(specs, elems, fills), dtypes

    def downsample_dev(self, elems, block, factor, d_blocks, d_out, stream=None, fills=None):
        """gf_block_downsample_elems_dev on device pointers: d_blocks[e] holds the rectangle block of element e (int32 / int16 /
        float32, row-major), d_out[e] receives the cells of downsample_rect(block, factor).  Enqueues only."""
        specs, _ = self._downsample_specs(elems, fills)
        ne = len(specs)
        assert len(d_blocks) == ne and len(d_out) == ne
        block = np.ascontiguousarray(block, np.int32)
        _call("gf_block_downsample_elems_dev", self._h, stream, _ptr(specs), ne, _ptr(block), int(factor), _ptrs(d_blocks), _ptrs(d_out))

    def downsample(self, elems, block, factor, blocks, fills=None):
        """gf_block_downsample_elems, the host-memory form (staged by the library): blocks[e] is the rectangle block of element e.
        Returns one array [n_rows', n_cols'] per element in the element's dtype, for downsample_rect(block, factor)."""
        specs, dtypes = self._downsample_specs(elems, fills)
        ne = len(specs)
        block = np.ascontiguousarray(block, np.int32)
        blocks = [np.ascontiguousarray(b, dt) for b, dt in zip(blocks, dtypes)]
        assert len(blocks) == ne and all(b.size == int(block[2]) * int(block[3]) for b in blocks)
        _, _, n_rows, n_cols = self.downsample_rect(block, factor)
        out = [np.zeros((n_rows, n_cols), dt) for dt in dtypes]
        _call("gf_block_downsample_elems", self._h, _ptr(specs), ne, _ptr(block), int(factor), _ptrs(blocks), _ptrs(out))
        return out

    # ---- a grid block tabulated: value counts, range and entropy (gf_block_tabulate_*, gf_tab_*) ----
    @staticmethod
    def tab_dense_plan(def_min, def_max, scale):
        """gf_tab_dense_plan_of: InputDataStatCollector's constructor -> dict n_counter, base, n_bins, scale_used"""
        spec, plan = _tab_dense_spec(def_min, def_max, scale), np.zeros(1, _TAB_DENSE_PLAN)
        _call("gf_tab_dense_plan_of", _ptr(spec), _ptr(plan))
        return {k: plan[k][0].item() for k in plan.dtype.names}

    def tabulate_dense_dev(self, elem_type, d_block, n_cells, def_min, def_max, scale, d_counter, d_summary, fill_i=0, skip_fill=False,
                           accumulate=False, first_cell=0, stream=None):
        """gf_block_tabulate_dense_dev on device pointers: n_cells cells of the element ("int", "short", "float" or GF_ELEM_*) ->
        d_counter [tab_dense_plan(...)["n_bins"]] int32 and d_summary, one gf_tab_summary (TAB_SUMMARY).  Enqueues only."""
        flags = (TAB_ACCUMULATE if accumulate else 0) | (TAB_SKIP_FILL if skip_fill else 0)
        spec = _tab_dense_spec(def_min, def_max, scale)
        _call("gf_block_tabulate_dense_dev", self._h, stream, _elem_type(elem_type), int(fill_i), flags, d_block, int(n_cells), int(first_cell),
              _ptr(spec), d_counter, d_summary)

    def tabulate_dense(self, elem_type, block, def_min, def_max, scale, fill_i=0, skip_fill=False, first_cell=0, into=None):
        """gf_block_tabulate_dense, the host-memory form (staged by the library): returns (counter [n_bins] int32, summary dict).
        into = (counter, summary) of an earlier call: accumulate onto them (a raster in strips, first_cell the strip's first cell)."""
        et = _elem_type(elem_type)
        block = np.ascontiguousarray(block, _delivered_dtype(et)).ravel()
        flags = (TAB_ACCUMULATE if into is not None else 0) | (TAB_SKIP_FILL if skip_fill else 0)
        summary = np.zeros(1, TAB_SUMMARY)
        if into is not None:
            counter = np.ascontiguousarray(into[0], np.int32).copy()
            for k in TAB_SUMMARY.names:
                summary[k] = into[1][k]
            assert counter.size == self.tab_dense_plan(def_min, def_max, scale)["n_bins"]
        else:
            counter = np.zeros(self.tab_dense_plan(def_min, def_max, scale)["n_bins"], np.int32)
        spec = _tab_dense_spec(def_min, def_max, scale)
        _call("gf_block_tabulate_dense", self._h, et, int(fill_i), flags, _ptr(block), block.size, int(first_cell), _ptr(spec), _ptr(counter),
              _ptr(summary))
        return counter, {k: summary[k][0].item() for k in TAB_SUMMARY.names}

    def tabulate_symbols_dev(self, elem_type, d_block, n_cells, d_symbols, d_counts, table_cap, d_summary, stream=None):
        """gf_block_tabulate_symbols_dev on device pointers: the distinct 32-bit symbols of n_cells cells in ascending unsigned order
        -> d_symbols [table_cap] uint32, d_counts [table_cap] int32 (both None with table_cap 0) and d_summary, one gf_tab_symbols
        (TAB_SYMBOLS).  Enqueues only."""
        _call("gf_block_tabulate_symbols_dev", self._h, stream, _elem_type(elem_type), d_block, int(n_cells), d_symbols, d_counts, int(table_cap),
              d_summary)

    def tabulate_symbols(self, elem_type, block, table_cap=None):
        """gf_block_tabulate_symbols, the host-memory form: returns (symbols uint32, counts int32, summary dict); table_cap None:
        room for every cell.  A table that does not hold every symbol comes back with its first table_cap entries (summary
        ["n_written"] of summary["n_symbols"])."""
        et = _elem_type(elem_type)
        block = np.ascontiguousarray(block, _delivered_dtype(et)).ravel()
        cap = block.size if table_cap is None else int(table_cap)
        symbols, counts, summary = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.int32), np.zeros(1, TAB_SYMBOLS)
        st = lib().gf_block_tabulate_symbols(self._h, et, _ptr(block), block.size, _ptr(symbols) if cap else None, _ptr(counts) if cap else None,
                                             cap, _ptr(summary))
        if st != _lib.ERR_CAPACITY:
            check(st, "gf_block_tabulate_symbols")
        n = int(summary["n_written"][0])
        return symbols[:n], counts[:n], {k: summary[k][0].item() for k in TAB_SYMBOLS.names}

    # ---- symbol tables merged, strips accumulated onto a table (gf_tab_symbols_merge[_dev], gf_block_tabulate_symbols_acc[_dev]) ----
    def tab_symbols_merge_dev(self, d_sym_a, d_cnt_a, d_sum_a, cap_a, d_sym_b, d_cnt_b, d_sum_b, cap_b, d_sym_out, d_cnt_out, table_cap, d_sum_out):
        """gf_tab_symbols_merge_dev on device pointers: tables A and B (their lengths are read on the device from their summaries:
        min(n_written, cap)) -> the out table, which overlaps neither.  Enqueues on the context's stream."""
        _call("gf_tab_symbols_merge_dev", self._h, d_sym_a, d_cnt_a, d_sum_a, int(cap_a), d_sym_b, d_cnt_b, d_sum_b, int(cap_b), d_sym_out,
              d_cnt_out, int(table_cap), d_sum_out)

    def tab_symbols_merge(self, a, b, table_cap=None):
        """gf_tab_symbols_merge, the host-memory form: a, b = (symbols, counts, summary dict) as tabulate_symbols returns them ->
        (symbols, counts, summary dict); table_cap None: room for every entry of both.  summary["reserved"] &
        TAB_SYM_INPUT_TRUNCATED: an input did not hold all of its symbols."""
        sa, ca, ua, arg_a = _tab_table_in(a)
        sb, cb, ub, arg_b = _tab_table_in(b)
        cap = sa.size + sb.size if table_cap is None else int(table_cap)
        fn = lib().gf_tab_symbols_merge
        return _tab_table_out("gf_tab_symbols_merge", cap, lambda sym, cnt, n, summ: fn(self._h, *arg_a, *arg_b, sym, cnt, n, summ))

    def tabulate_symbols_acc_dev(self, elem_type, d_block, n_cells, d_sym_in, d_cnt_in, d_sum_in, cap_in, d_sym_out, d_cnt_out, cap_out, d_sum_out):
        """gf_block_tabulate_symbols_acc_dev on device pointers: the symbols of n_cells cells (a strip of a raster) counted onto the
        in-table (None / cap_in 0: empty) -> the out table, which does not overlap it.  Enqueues on the context's stream."""
        _call("gf_block_tabulate_symbols_acc_dev", self._h, _elem_type(elem_type), d_block, int(n_cells), d_sym_in, d_cnt_in, d_sum_in, int(cap_in),
              d_sym_out, d_cnt_out, int(cap_out), d_sum_out)

    def tabulate_symbols_acc(self, elem_type, block, into=None, table_cap=None):
        """gf_block_tabulate_symbols_acc, the host-memory form: the symbols of block counted onto the table into = (symbols, counts,
        summary dict) of an earlier call (None: empty) -> (symbols, counts, summary dict); table_cap None: room for every cell."""
        et = _elem_type(elem_type)
        block = np.ascontiguousarray(block, _delivered_dtype(et)).ravel()
        keep = block if block.size else np.zeros(1, block.dtype)
        si, ci, ui, arg_in = _tab_table_in(into)
        cap = arg_in[3] + block.size if table_cap is None else int(table_cap)
        fn = lib().gf_block_tabulate_symbols_acc
        return _tab_table_out("gf_block_tabulate_symbols_acc", cap,
                              lambda sym, cnt, n, summ: fn(self._h, et, _ptr(keep), block.size, *arg_in, sym, cnt, n, summ))

    @staticmethod
    def tab_entropy(counts, n_samples, kahan=True):
        """gf_tab_entropy_counts: bits per sample of a table of counts in the order given; kahan: EntropyTabulator's sum, else
        InputDataStatCollector.getEntropy's"""
        counts, e = np.ascontiguousarray(counts, np.int32).ravel(), C.c_double()
        _call("gf_tab_entropy_counts", _ptr(counts), counts.size, int(n_samples), int(bool(kahan)), C.byref(e))
        return e.value

    # ---- ARGB images as element planes and as overviews (gf_image_split / _join / _reduce) ----
    @staticmethod
    def _image_kind(model, elem_type):
        """(GF_IMAGE_*, GF_ELEM_*, the planes' dtype) of a model's and an element's name or number; planes are "int" or "short" """
        model, et = (IMAGE_MODELS[model] if isinstance(model, str) else int(model)), _elem_type(elem_type)
        return model, et, _ELEM_KINDS["short" if et == ELEM_TYPES["short"] else "int"].delivered

    def image_split_dev(self, model, elem_type, n_pixels, d_argb, d_planes):
        """gf_image_split_dev on device pointers: n_pixels ARGB words -> three planes (model "rgb": r, g, b; "ycocg": Y, Co, Cg) of
        int32 ("int") or int16 ("short").  Runs on the context's stream; enqueues only."""
        model, et, _ = self._image_kind(model, elem_type)
        assert len(d_planes) == 3
        _call("gf_image_split_dev", self._h, model, et, int(n_pixels), d_argb, _ptrs(d_planes))

    def image_join_dev(self, model, elem_type, n_pixels, d_planes, d_argb):
        """gf_image_join_dev, the inverse: three planes of any ints -> n_pixels ARGB words.  Enqueues only."""
        model, et, _ = self._image_kind(model, elem_type)
        assert len(d_planes) == 3
        _call("gf_image_join_dev", self._h, model, et, int(n_pixels), _ptrs(d_planes), d_argb)

    @staticmethod
    def image_reduce_size(width, height, factor):
        """gf_image_reduce_size: (width // factor, height // factor)"""
        w, h = C.c_int(), C.c_int()
        _call("gf_image_reduce_size", int(width), int(height), int(factor), C.byref(w), C.byref(h))
        return w.value, h.value

    def image_reduce_dev(self, width, height, factor, d_argb, d_out):
        """gf_image_reduce_dev: height rows of width ARGB words -> the image of image_reduce_size(...), each word the per-channel
        box average of factor x factor pixels as DemoCOG.makeReducedImage rounds it.  Enqueues only."""
        _call("gf_image_reduce_dev", self._h, int(width), int(height), int(factor), d_argb, d_out)

    def image_split(self, argb, model="ycocg", elem_type="short"):
        """gf_image_split, the host-memory form (staged by the library): three planes in the shape of argb"""
        model, et, dt = self._image_kind(model, elem_type)
        argb = _argb_words(argb)
        planes = [np.zeros(argb.shape, dt) for _ in range(3)]
        _call("gf_image_split", self._h, model, et, argb.size, _ptr(argb), _ptrs(planes))
        return planes

    def image_join(self, planes, model="ycocg", elem_type="short"):
        """gf_image_join, the host-memory form: ARGB words (int32) in the shape of the planes"""
        model, et, dt = self._image_kind(model, elem_type)
        planes = [np.ascontiguousarray(p, dt) for p in planes]
        assert len(planes) == 3 and all(p.shape == planes[0].shape for p in planes)
        argb = np.zeros(planes[0].shape, np.int32)
        _call("gf_image_join", self._h, model, et, argb.size, _ptrs(planes), _ptr(argb))
        return argb

    def image_reduce(self, argb, factor):
        """gf_image_reduce, the host-memory form: argb [height, width] -> int32 [height // factor, width // factor]"""
        argb = _argb_words(argb)
        assert argb.ndim == 2
        w, h = self.image_reduce_size(argb.shape[1], argb.shape[0], factor)
        out = np.zeros((h, w), np.int32)
        _call("gf_image_reduce", self._h, argb.shape[1], argb.shape[0], int(factor), _ptr(argb), _ptr(out))
        return out

    def close(self):
        if self._h:
            lib().gf_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Palette:
    """A colour palette on a context's device (gf_palette_create): what the reference's ColorPaletteTable holds.  records as
    palette_records() takes them; the other arguments are the table constructor's."""

    def __init__(self, ctx, records, argb_for_null=0, normalized=False, range_min=0.0, range_max=0.0, hinge=False, hinge_value=0.0):
        self._h = C.c_void_p()
        spec, recs = palette_spec(records, argb_for_null, normalized, range_min, range_max, hinge, hinge_value)
        _call("gf_palette_create", ctx.handle, _ptr(spec), C.byref(self._h))
        self.ctx, self.n_records = ctx, len(recs)

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib().gf_palette_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceTileBatch:
    """Device-resident batch of tiles and their packings: the measured hot path.

    encode(): values -> slots/lengths/predictors/status   (gf_huffman_encode_batch_i32_dev)
    decode(): slots/lengths -> decoded/status              (gf_huffman_decode_batch_i32_dev)
    Nothing synchronises unless asked; everything is enqueued on `stream` (default: the
    context's stream).
    """

    def __init__(self, ctx, n_rows, n_cols, n_tiles, slot_stride=None, codec="huffman"):
        assert codec in ("huffman", "canon", "lsop")
        self.codec = codec
        self.ctx, self.n_rows, self.n_cols, self.n_tiles = ctx, int(n_rows), int(n_cols), int(n_tiles)
        self.cells = self.n_rows * self.n_cols
        self.stride = int(slot_stride or lib().gf_huffman_default_stride(n_rows, n_cols))
        assert self.stride % 16 == 0
        nt = self.n_tiles
        self.values = DeviceBuffer(ctx, nt * self.cells * 4)
        self.decoded = DeviceBuffer(ctx, nt * self.cells * 4)
        self.slots = DeviceBuffer(ctx, nt * self.stride + 16)
        self.lengths = DeviceBuffer(ctx, nt * 4)
        self.predictors = DeviceBuffer(ctx, nt)
        self.enc_status = DeviceBuffer(ctx, nt * 4)
        self.dec_status = DeviceBuffer(ctx, nt * 4)
        self._buffers = [self.values, self.decoded, self.slots, self.lengths, self.predictors, self.enc_status, self.dec_status]
        ctx.reserve(n_rows, n_cols, nt)
        if codec == "lsop":                          # work buffers of the LSOP stages
            n = int(lib().gf_lsop12_residual_count(n_rows, n_cols))
            self.res_stride = (n + 3) // 4 * 4
            self.residuals = DeviceBuffer(ctx, nt * self.res_stride * 4 + 16)
            self.coefs = DeviceBuffer(ctx, nt * 64)
            self.scratch_status = DeviceBuffer(ctx, nt * 4)
            self._buffers += [self.residuals, self.coefs, self.scratch_status]

    def synth_dem(self, seed, tiles_per_row, tile0=0, stream=None, mask_per_mille=0, style=0):
        head = (self.ctx.handle, stream, seed & (2 ** 64 - 1), self.n_rows, self.n_cols, tiles_per_row, tile0, self.n_tiles)
        if style:
            _call("gf_synth_dem_style_dev", *head, mask_per_mille, style, self.values.ptr)
        elif mask_per_mille:
            _call("gf_synth_dem_masked_dev", *head, mask_per_mille, self.values.ptr)
        else:
            _call("gf_synth_dem_dev", *head, self.values.ptr)

    def encode(self, codec_index=0, predictor_mask=_lib.PM_ALL, stream=None, lsop_flags=0):
        if self.codec == "lsop":
            _call("gf_lsop12_encode_batch_i32_dev_ex", self.ctx.handle, stream, codec_index, self.n_rows, self.n_cols, self.n_tiles,
                  self.values.ptr, lsop_flags, self.slots.ptr, self.stride, self.lengths.ptr, self.enc_status.ptr, self.residuals.ptr,
                  self.res_stride, self.coefs.ptr, self.scratch_status.ptr)
            return
        _call("gf_%s_encode_batch_i32_dev" % self.codec, self.ctx.handle, stream, codec_index, self.n_rows, self.n_cols, self.n_tiles,
              self.values.ptr, self.slots.ptr, self.stride, self.lengths.ptr, self.predictors.ptr, self.enc_status.ptr, predictor_mask)

    def decode(self, stream=None):
        if self.codec == "lsop":
            _call("gf_lsop12_decode_batch_i32_dev", self.ctx.handle, stream, self.n_rows, self.n_cols, self.n_tiles, self.slots.ptr,
                  self.n_tiles * self.stride, None, self.stride, self.lengths.ptr, self.decoded.ptr, self.dec_status.ptr,
                  self.residuals.ptr, self.res_stride, self.coefs.ptr, self.scratch_status.ptr)
            return
        _call("gf_%s_decode_batch_i32_dev" % self.codec, self.ctx.handle, stream, self.n_rows, self.n_cols, self.n_tiles, self.slots.ptr,
              self.n_tiles * self.stride, None, self.stride, self.lengths.ptr, self.decoded.ptr, self.dec_status.ptr)

    # host views (synchronising copies)
    def get_lengths(self):
        return self.lengths.download(np.uint32, self.n_tiles)

    def get_predictors(self):
        return self.predictors.download(np.uint8, self.n_tiles)

    def get_enc_status(self):
        return self.enc_status.download(np.int32, self.n_tiles)

    def get_dec_status(self):
        return self.dec_status.download(np.int32, self.n_tiles)

    def get_packing(self, t, length=None):
        if length is None:
            length = int(self.lengths.download(np.uint32, 1, 4 * t)[0])
        return bytes(self.slots.download(np.uint8, length, t * self.stride))

    def get_values(self, t0=0, n=None):
        n = self.n_tiles - t0 if n is None else n
        return self.values.download(np.int32, n * self.cells, t0 * self.cells * 4).reshape(n, self.cells)

    def get_decoded(self, t0=0, n=None):
        n = self.n_tiles - t0 if n is None else n
        return self.decoded.download(np.int32, n * self.cells, t0 * self.cells * 4).reshape(n, self.cells)

    def free(self):
        """Frees every buffer of the batch, the LSOP work buffers included."""
        for b in self._buffers:
            b.free()


class GpuTimer:
    """HIP-event timer on the stream the kernels are launched on (gf_timer_*)."""

    def __init__(self, ctx):
        self._h = C.c_void_p()
        _call("gf_timer_create", ctx.handle, C.byref(self._h))

    def start(self, stream=None):
        _call("gf_timer_start", self._h, stream)

    def stop(self, stream=None):
        _call("gf_timer_stop", self._h, stream)

    def elapsed_ms(self):
        ms = C.c_float(0)
        _call("gf_timer_elapsed_ms", self._h, C.byref(ms))
        return ms.value

    def __del__(self):
        try:
            if self._h:
                lib().gf_timer_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


# ---- the codec classes ----
class CodecHuffmanHip:
    """Drop-in for org.gridfour.compress.CodecHuffman, computed on the MI355X."""

    _PREFIX = "gf_huffman"                       # entry-point family of the C ABI

    def __init__(self, context=None, device=0):
        self.ctx = context if context is not None else GvrsHipContext(device)

    def _fn(self, name):
        return getattr(lib(), "%s_%s" % (self._PREFIX, name))

    # ---- ICompressionEncoder ----
    def encode(self, codecIndex, nRows, nCols, values):
        v = np.ascontiguousarray(values, dtype=np.int32).ravel()
        if v.size != nRows * nCols:
            raise ValueError("values.length != nRows*nCols")
        cap = int(self._fn("max_packing")(nRows, nCols))
        out = np.empty(cap, np.uint8)
        n = C.c_size_t(0)
        st = self._fn("encode_i32")(self.ctx.handle, codecIndex, nRows, nCols, _ptr(v), _ptr(out), cap, C.byref(n))
        if st == _lib.DECLINED:
            return None
        if st == _lib.ERR_BOUNDS:
            raise IndexError("ArrayIndexOutOfBoundsException in the reference for these dimensions")
        if st == _lib.ERR_ARG and self._PREFIX == "gf_canon":
            raise ValueError("IllegalArgumentException in the reference for these dimensions")
        check(st, self._PREFIX + "_encode_i32")
        return bytes(out[:n.value])

    def encodeFloats(self, codecIndex, nRows, nCols, values):
        return None                                  # CodecHuffman.java:237-239

    def implementsFloatingPointEncoding(self):
        return False

    def implementsIntegerEncoding(self):
        return True

    # ---- ICompressionDecoder ----
    def decode(self, nRows, nColumns, packing):
        p = np.frombuffer(bytes(packing), dtype=np.uint8)
        out = np.empty(nRows * nColumns, np.int32)
        st = self._fn("decode_i32")(self.ctx.handle, nRows, nColumns, _ptr(p), p.size, _ptr(out))
        if st in (_lib.ERR_FORMAT, _lib.ERR_BOUNDS):
            raise IOError(lib().gf_status_string(st).decode())
        if st == _lib.DECLINED:                      # CodecDeflate.decode: the inflater gave nothing -> null (:143-154)
            return None
        check(st, self._PREFIX + "_decode_i32")
        return out

    def decodeFloats(self, nRows, nColumns, packing):
        return None                                  # CodecHuffman.java:242-244

    # ---- analysis (CodecHuffman.java:172-234 over CodecStats.java) ----
    _STAT_LABELS = ("None", "Differencing", "Linear", "Triangle", "DifferencingWithNulls", "All Predictors")

    def analyze(self, nRows, nColumns, packing):
        st = self.analyze_batch(nRows, nColumns, [packing])
        if st[0] != 0:
            raise IOError(lib().gf_status_string(int(st[0])).decode())

    def analyze_batch(self, nRows, nCols, packings):
        """analyze() of every packing in one GPU pass; returns the per-packing status (non-zero: analyze would throw)."""
        if self._PREFIX != "gf_huffman":
            raise NotImplementedError("statistics are gathered for CodecHuffman only")
        if getattr(self, "_stats", None) is None:
            self._stats = np.zeros(6, dtype=CODEC_STATS_DTYPE)
        nt = len(packings)
        blob, offsets = _blob_of(packings)
        status = np.zeros(nt, np.int32)
        if getattr(self, "_pairs", None) is None:
            self._pairs = np.zeros((6, 65536), np.int64)          # sB of the six CodecStats (CodecStats.java:64)
        _call("gf_huffman_analyze_batch_h2", self.ctx.handle, nRows, nCols, nt, _ptr(blob), _ptr(offsets), _ptr(self._stats), _ptr(self._pairs),
              _ptr(status))
        return status

    def pair_counts(self):
        """sB[(prior << 8) | value] of the six CodecStats (five predictors, all)."""
        p = getattr(self, "_pairs", None)
        return None if p is None else p.copy()

    def getH2(self, k=5):
        """CodecStats.getH2 of record k (0..4 by predictor code, 5 = all predictors)."""
        p = getattr(self, "_pairs", None)
        return 0.0 if p is None else float(lib().gf_codec_stats_h2(_ptr(np.ascontiguousarray(p[k]))))

    def analysis_data(self):
        """The accumulated sums, one record per predictor code 0..4 and one for all (CodecStats fields)."""
        s = getattr(self, "_stats", None)
        return None if s is None else s.copy()

    def reportAnalysisData(self, ps, nTilesInRaster):
        ps.write("Gridfour_Huffman                               Compressed Output    |       Predictor Residuals\n")
        s = getattr(self, "_stats", None)
        if s is None or nTilesInRaster == 0:
            ps.write("   Tiles Compressed:  0\n")
            return
        ps.write("  Predictor                Times Used        bits/sym    bits/tile  |  m32 avg-len   avg-unique  entropy | bits in tree\n")
        for label, r in zip(self._STAT_LABELS, s):
            if label == "None":
                continue
            n, nm = int(r["n_tiles"]), int(r["n_m32_counted"])
            bits_per_symbol = 8.0 * r["n_bytes"] / r["n_symbols"] if r["n_symbols"] else 0.0
            ps.write("   %-20.20s %8d (%4.1f %%)     %5.2f  %12.1f   | %10.1f      %6.1f    %6.2f   | %6.1f\n" % (
                label, n, 100.0 * n / nTilesInRaster, bits_per_symbol, (r["n_bytes"] / n * 8 if n else 0.0),
                (r["sum_length_m32"] / nm if nm else 0.0), (r["sum_observed_m32"] / n if n else 0.0),
                (r["sum_entropy_m32"] / nm if nm else 0.0), (r["n_bits_overhead"] / n if n else 0.0)))

    def clearAnalysisData(self):
        self._stats = None
        self._pairs = None

    # ---- batched forms (host memory) ----
    def encode_batch(self, codecIndex, nRows, nCols, tiles):
        """tiles: int32 [nTiles, nRows*nCols].  Returns (packings: list[bytes|None], predictors, status)."""
        v = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, nRows * nCols)
        nt = v.shape[0]
        offsets = np.zeros(nt + 1, np.uint64)
        preds = np.zeros(nt, np.uint8)
        status = np.zeros(nt, np.int32)
        fn = self._fn("encode_batch_i32")
        st, blob = _grown_blob(lambda blob, cap: fn(self.ctx.handle, codecIndex, nRows, nCols, nt, _ptr(v), _ptr(blob), cap, _ptr(offsets),
                                                    _ptr(preds), _ptr(status)),
                               nt * int(lib().gf_huffman_default_stride(nRows, nCols)), 16, offsets)
        check(st, self._PREFIX + "_encode_batch_i32")
        return _records_out(blob, offsets, nt, status), preds, status

    def decode_batch(self, nRows, nCols, packings):
        """packings: list of bytes.  Returns (values int32 [nTiles, cells], status)."""
        nt = len(packings)
        blob, offsets = _blob_of(packings)
        out = np.empty((nt, nRows * nCols), np.int32)
        status = np.zeros(nt, np.int32)
        _call(self._PREFIX + "_decode_batch_i32", self.ctx.handle, nRows, nCols, nt, _ptr(blob), _ptr(offsets), _ptr(out), _ptr(status))
        return out, status


class CodecDeflateHip(CodecHuffmanHip):
    """Drop-in for org.gridfour.compress.CodecDeflate: predictor + CodecM32 on the MI355X, Deflate (level 6) on the host's
    zlib as the reference uses the JDK's."""

    _PREFIX = "gf_deflate"

    def _fn(self, name):
        if name == "max_packing":                    # nM32 + 128 bytes at most (CodecDeflate.java:204)
            return lambda r, c: int(lib().gf_m32_max_stream(r, c)) + 256
        return getattr(lib(), "%s_%s" % (self._PREFIX, name))


class CodecCanonHuffmanHip(CodecHuffmanHip):
    """Drop-in for org.gridfour.compress.canonicalHuffman.CodecCanonHuffman (the default integer codec of
    current Gridfour, GvrsFileSpecification.java:229), computed on the MI355X."""

    _PREFIX = "gf_canon"

    # ---- analysis (CodecCanonHuffman.java:217-324 over CanonHuffmanStats.java) ----
    _ESCAPE_BITS = (2, 4, 6, 8, 16, 24)                  # CanonicalHuffman.getEscapeBitCounts()[0]

    def analyze(self, nRows, nColumns, packing):
        st = self.analyze_batch(nRows, nColumns, [packing])
        if st[0] != 0:
            raise IOError(lib().gf_status_string(int(st[0])).decode())

    def analyze_batch(self, nRows, nCols, packings):
        """analyze() of every packing in one GPU pass; returns the per-packing status (non-zero: analyze would throw)."""
        nt = len(packings)
        status = np.zeros(nt, np.int32)
        if nt == 0:
            return status
        if getattr(self, "_stats", None) is None:
            self._stats = np.zeros(6, dtype=CANON_STATS_DTYPE)
            self._escapes = np.zeros(6, np.int64)
        blob, offsets = _blob_of(packings)
        _call("gf_canon_analyze_batch", self.ctx.handle, nRows, nCols, nt, _ptr(blob), _ptr(offsets), _ptr(self._stats), _ptr(self._escapes),
              _ptr(status))
        return status

    def analysis_data(self):
        """The accumulated sums, one record per predictor byte 0..4 (0: the uniform form) and one for all (CanonHuffmanStats fields)."""
        s = getattr(self, "_stats", None)
        return None if s is None else s.copy()

    def escape_counts(self):
        """escapeBitCounts[1]: how many values took 2, 4, 6, 8, 16, 24 escape bits."""
        e = getattr(self, "_escapes", None)
        return None if e is None else e.copy()

    def reportAnalysisData(self, ps, nTilesInRaster):
        ps.write("GVRS Canonical Huffman                          Compressed Output    |       Predictor Residuals\n")
        s = getattr(self, "_stats", None)
        if s is None or nTilesInRaster == 0:
            ps.write("   Tiles Compressed:  0\n")
            return
        ps.write("  Predictor                Times Used         bits/sym    bits/tile  |    ext-bits    avg-unique  entropy | bits in tree\n")
        for label, r in zip(self._STAT_LABELS, s):
            if label == "None":
                label = "Uniform Value"                  # the uniform case is counted under predictor code 0
                if r["n_tiles"] == 0:
                    continue
            n, nt = int(r["n_tiles"]), int(r["n_text_counted"])
            line_label = "%-20.20s %8d (%4.1f %%)" % (label, n, 100.0 * n / nTilesInRaster)
            ps.write("   %-39.39s     %5.2f  %12.1f   | %10.1f      %6.1f    %6.2f   | %6.1f\n" % (
                line_label, (8.0 * r["n_bytes"] / r["n_symbols"] if r["n_symbols"] else 0.0),
                (r["n_bytes"] / n * 8 if n else 0.0), (r["sum_escape_bits"] / n if n else 0.0),
                (r["sum_observed"] / n if n else 0.0), (r["sum_entropy"] / nt if nt else 0.0),
                (r["n_bits_overhead"] / n if n else 0.0)))
        total = float(s[5]["n_tiles"])
        if total <= 0:
            total = 1.0                                  # just for averaging
        ps.write("Escape sequences\n")
        ps.write("length    count     n/tile  bits/tile\n")
        for bits, count in zip(self._ESCAPE_BITS, self._escapes):
            ps.write("  %2d  %10d    %7.2f    %7.2f\n" % (bits, count, count / total, bits * (count / total)))

    def clearAnalysisData(self):
        self._stats = None
        self._escapes = None


class CodecFloatHip:
    """Drop-in for org.gridfour.compress.CodecFloat (CodecFloat.java:328-458): float32 tiles as five
    byte planes (split/merged on the GPU) each compressed with zlib on the host.

    `level` is the zlib level: 9 is what the current reference source passes to java.util.zip.Deflater,
    6 is what the reference's sample files were written with."""

    def __init__(self, context=None, device=0, level=9):
        self.ctx = context if context is not None else GvrsHipContext(device)
        self.level = int(level)

    # ---- ICompressionEncoder ----
    def encode(self, codecIndex, nRows, nCols, values):
        return None                                  # CodecFloat.java: integer encoding not implemented

    def encodeFloats(self, codecIndex, nRows, nCols, values):
        v = np.ascontiguousarray(values, dtype=np.float32).ravel()
        if v.size != nRows * nCols:
            raise ValueError("values.length != nRows*nCols")
        cap = 5 * v.size + 4096
        out = np.empty(cap, np.uint8)
        n = C.c_size_t(0)
        _call("gf_float_encode_f32", self.ctx.handle, codecIndex, nRows, nCols, _ptr(v), self.level, _ptr(out), cap, C.byref(n))
        return bytes(out[:n.value])

    def implementsFloatingPointEncoding(self):
        return True

    def implementsIntegerEncoding(self):
        return False

    # ---- ICompressionDecoder ----
    def decode(self, nRows, nColumns, packing):
        return None

    def decodeFloats(self, nRows, nColumns, packing):
        p = np.frombuffer(bytes(packing), dtype=np.uint8)
        out = np.empty(nRows * nColumns, np.float32)
        st = lib().gf_float_decode_f32(self.ctx.handle, nRows, nColumns, _ptr(p), p.size, _ptr(out))
        if st in (_lib.ERR_FORMAT, _lib.ERR_BOUNDS):
            raise IOError(lib().gf_status_string(st).decode())
        check(st, "gf_float_decode_f32")
        return out

    # ---- batched, host memory ----
    def encode_floats_batch(self, codecIndex, nRows, nCols, tiles):
        v = np.ascontiguousarray(tiles, dtype=np.float32).reshape(-1, nRows * nCols)
        nt = v.shape[0]
        cap = nt * (5 * nRows * nCols + 4096)
        blob = np.empty(cap, np.uint8)
        offsets = np.zeros(nt + 1, np.uint64)
        _call("gf_float_encode_batch_f32", self.ctx.handle, codecIndex, nRows, nCols, nt, _ptr(v), self.level, _ptr(blob), cap, _ptr(offsets))
        return _records_out(blob, offsets, nt)

    def decode_floats_batch(self, nRows, nCols, packings):
        nt = len(packings)
        blob, offsets = _blob_of(packings)
        out = np.empty((nt, nRows * nCols), np.float32)
        status = np.zeros(nt, np.int32)
        _call("gf_float_decode_batch_f32", self.ctx.handle, nRows, nCols, nt, _ptr(blob), _ptr(offsets), _ptr(out), _ptr(status))
        return out, status


class _LsCodecBase:
    """What the two optimal-predictor codecs share: the ICompressionEncoder / ICompressionDecoder forms, the batched host forms and
    the predictor stage alone.  A subclass names its entry points' prefix (_PREFIX), its coefficient count (_N_COEF), the arguments
    its device forms take between the context and the shape (_DEV_HEAD).  The docstrings cite the reference classes of both:
    org.gridfour.lsop.LsEncoder12 / LsDecoder12 / LsOptimalPredictor12 and their 08 siblings."""
    _PREFIX, _N_COEF, _DEV_HEAD = None, 0, ()

    def __init__(self, context=None, device=0):
        self.ctx = context if context is not None else GvrsHipContext(device)

    def _encode_flags(self):
        """the arguments of <prefix>_encode_batch_i32 between the values and the blob"""
        return ()

    # ---- ICompressionEncoder ----
    def encode(self, codecIndex, nRows, nCols, values):
        packs, _, status = self.encode_batch(codecIndex, nRows, nCols, np.asarray(values).reshape(1, -1))
        if status[0] == _lib.DECLINED:
            return None
        check(int(status[0]), self._PREFIX + "_encode_batch_i32")
        return packs[0]

    def encodeFloats(self, codecIndex, nRows, nCols, values):
        return None                                             # LsEncoder12.java:222-224, LsEncoder08.java:140-142

    def implementsFloatingPointEncoding(self):
        return False

    def implementsIntegerEncoding(self):
        return True

    # ---- ICompressionDecoder ----
    def decode(self, nRows, nColumns, packing):
        vals, status = self.decode_batch(nRows, nColumns, [packing])
        if status[0] in (_lib.ERR_FORMAT, _lib.ERR_BOUNDS):
            raise IOError(lib().gf_status_string(int(status[0])).decode())
        check(int(status[0]), self._PREFIX + "_decode_batch_i32")
        return vals[0]

    def decodeFloats(self, nRows, nColumns, packing):
        return None

    # ---- batched forms (host memory) ----
    def encode_batch(self, codecIndex, nRows, nCols, tiles):
        """Returns (packings: list[bytes|None], container types uint8, status int32)."""
        v = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, nRows * nCols)
        nt = v.shape[0]
        cap = nt * int(getattr(lib(), self._PREFIX + "_max_packing")(nRows, nCols)) + 64
        blob = np.empty(cap, np.uint8)
        offsets = np.zeros(nt + 1, np.uint64)
        types = np.zeros(nt, np.uint8)
        status = np.zeros(nt, np.int32)
        _call(self._PREFIX + "_encode_batch_i32", self.ctx.handle, codecIndex, nRows, nCols, nt, _ptr(v), *self._encode_flags(), _ptr(blob), cap,
              _ptr(offsets), _ptr(types), _ptr(status))
        return _records_out(blob, offsets, nt, status), types, status

    def decode_batch(self, nRows, nCols, packings):
        nt = len(packings)
        blob, offsets = _blob_of(packings)
        out = np.zeros((nt, nRows * nCols), np.int32)
        status = np.zeros(nt, np.int32)
        _call(self._PREFIX + "_decode_batch_i32", self.ctx.handle, nRows, nCols, nt, _ptr(blob), _ptr(offsets), _ptr(out), _ptr(status))
        return out, status

    # ---- the predictor stage alone (device buffers handled here; used by tests and tools) ----
    def _strides(self, nRows, nCols):
        n = int(getattr(lib(), self._PREFIX + "_residual_count")(nRows, nCols))
        return n, max(4, (n + 3) // 4 * 4)

    def predict(self, nRows, nCols, tiles):
        """LsOptimalPredictor12 / 08.encode: returns (seed, coefficients float32[nt, 12 or 8], residuals int32[nt,n], status)."""
        v = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, nRows * nCols)
        nt = v.shape[0]
        n, stride = self._strides(nRows, nCols)
        with _DeviceScope(self.ctx) as s:
            dv, dr, dc, ds = s.upload(v), s.alloc(nt * stride * 4 + 16), s.alloc(nt * 64, fill=0), s.alloc(nt * 4)
            s.run(self._PREFIX + "_predict_dev", self.ctx.handle, *self._DEV_HEAD, nRows, nCols, nt, dv.ptr, dr.ptr, stride, dc.ptr, ds.ptr)
            res = dr.download(np.int32, nt * stride).reshape(nt, stride)[:, :n]
            coefs = dc.download(np.uint32, nt * 16).reshape(nt, 16)
            status = ds.download(np.int32, nt)
        return coefs[:, 0].astype(np.int32), coefs[:, 1:1 + self._N_COEF].copy().view(np.float32), res, status

    def reconstruct(self, nRows, nCols, seeds, coefficients, residuals):
        """LsDecoder12 / 08.unpackInitializers/unpackInterior: returns (values int32[nt, cells], status)."""
        res = np.ascontiguousarray(residuals, dtype=np.int32)
        nt, n = res.shape
        stride = max(4, (n + 3) // 4 * 4)
        padded = np.zeros((nt, stride), np.int32)
        padded[:, :n] = res
        coefs = np.zeros((nt, 16), np.uint32)
        coefs[:, 0] = np.asarray(seeds, np.int32).view(np.uint32)
        coefs[:, 1:1 + self._N_COEF] = np.ascontiguousarray(coefficients, np.float32).view(np.uint32).reshape(nt, self._N_COEF)
        with _DeviceScope(self.ctx) as s:
            dv, dr, dc, ds = s.alloc(nt * nRows * nCols * 4), s.upload(padded, slack=16), s.upload(coefs), s.alloc(nt * 4)
            s.run(self._PREFIX + "_reconstruct_dev", self.ctx.handle, *self._DEV_HEAD, nRows, nCols, nt, dr.ptr, stride, dc.ptr, None, dv.ptr,
                  ds.ptr)
            vals = dv.download(np.int32, nt * nRows * nCols).reshape(nt, nRows * nCols)
            status = ds.download(np.int32, nt)
        return vals, status


class LsCodecHip(_LsCodecBase):
    """Drop-in for org.gridfour.lsop.LsEncoder12 + LsDecoder12 (codec id "LSOP12", LsCodecUtility.java:53),
    computed on the MI355X; the Deflate alternative container uses the host's zlib as the reference uses the JDK's."""
    _PREFIX, _N_COEF, _DEV_HEAD = "gf_lsop12", 12, (None,)      # (its device forms take a stream: the context's own)

    def __init__(self, context=None, device=0, deflate_enabled=True, value_checksum_enabled=False):
        super().__init__(context, device)
        self.deflate_enabled = bool(deflate_enabled)           # LsEncoder12.setDeflateEnabled, default true
        self.value_checksum_enabled = bool(value_checksum_enabled)   # LsEncoder12.setValueChecksumEnabled, default false

    def setDeflateEnabled(self, enabled):
        self.deflate_enabled = bool(enabled)

    def setValueChecksumEnabled(self, enabled):
        self.value_checksum_enabled = bool(enabled)            # LsEncoder12.java:117-119

    def _encode_flags(self):
        return ((_lib.LSOP_DEFLATE if self.deflate_enabled else 0) | (_lib.LSOP_VALUE_CHECKSUM if self.value_checksum_enabled else 0),)


class LsCodec08Hip(_LsCodecBase):
    """Drop-in for org.gridfour.lsop.LsEncoder08 + LsDecoder08 (codec id "LSOP08", the 3 x 3-neighbourhood sibling of LSOP12), computed
    on the MI355X.  encode / encode_batch give the reference's choice between the Huffman and the Deflate container (the latter with
    the host's zlib, as the reference uses the JDK's); encode_batch_dev is the device encoder, which writes the Huffman container."""
    _PREFIX, _N_COEF = "gf_lsop08", 8

    # ---- the device forms (device buffers handled here; used by tests and tools) ----
    def encode_batch_dev(self, codecIndex, nRows, nCols, tiles):
        """gf_lsop08_encode_batch_i32_dev: the Huffman container of every tile.  Returns (packings: list[bytes|None], status)."""
        v = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, nRows * nCols)
        nt = v.shape[0]
        _, stride = self._strides(nRows, nCols)
        slot = max(64, int(lib().gf_lsop08_max_packing(nRows, nCols)))
        with _DeviceScope(self.ctx) as s:
            dv, do, dl, ds = s.upload(v), s.alloc(nt * slot + 16), s.alloc(nt * 4), s.alloc(nt * 4)
            dr, dc, d2 = s.alloc(nt * stride * 4 + 16), s.alloc(nt * 64), s.alloc(nt * 4)
            s.run("gf_lsop08_encode_batch_i32_dev", self.ctx.handle, codecIndex, nRows, nCols, nt, dv.ptr, do.ptr, slot, dl.ptr, ds.ptr,
                  dr.ptr, stride, dc.ptr, d2.ptr)
            status = ds.download(np.int32, nt)
            lengths = dl.download(np.uint32, nt)
            slots = do.download(np.uint8, nt * slot).reshape(nt, slot)
        return [bytes(slots[t, :lengths[t]]) if status[t] == _lib.OK else None for t in range(nt)], status

    def decode_batch_dev(self, nRows, nCols, packings):
        """gf_lsop08_decode_batch_i32_dev on packings laid back to back in device memory.  Returns (values, status)."""
        nt = len(packings)
        blob, offsets = _blob_of(packings)
        lengths = np.diff(offsets).astype(np.uint32)
        _, stride = self._strides(nRows, nCols)
        with _DeviceScope(self.ctx) as s:
            db, dof, dl = s.upload(blob, slack=16), s.upload(offsets), s.upload(lengths)
            dv, ds = s.alloc(nt * nRows * nCols * 4), s.alloc(nt * 4)
            dr, dc, d2 = s.alloc(nt * stride * 4 + 16), s.alloc(nt * 64), s.alloc(nt * 4)
            s.run("gf_lsop08_decode_batch_i32_dev", self.ctx.handle, nRows, nCols, nt, db.ptr, int(offsets[-1]), dof.ptr, 0, dl.ptr, dv.ptr,
                  ds.ptr, dr.ptr, stride, dc.ptr, d2.ptr)
            vals = dv.download(np.int32, nt * nRows * nCols).reshape(nt, nRows * nCols)
            status = ds.download(np.int32, nt)
        return vals, status


class CodecMasterHip:
    """org.gridfour.gvrs.CodecMaster over a codec list, batched: the strictly shortest packing per tile (list order
    breaks ties), decode dispatch on packing[0]."""

    def __init__(self, codec_list=STANDARD_CODEC_LIST, context=None, device=0):
        self.ctx = context if context is not None else GvrsHipContext(device)
        self.codecs = np.asarray(codec_list, dtype=np.int32)

    def _codecs_arg(self):
        return self.codecs if self.codecs.size else np.zeros(1, np.int32)

    def _head(self, stream=False):
        """The arguments every entry point over a codec list begins with: the context, with stream the NULL stream, the list"""
        return (self.ctx.handle,) + ((None,) if stream else ()) + (_ptr(self._codecs_arg()), self.codecs.size)

    def encode_batch(self, nRows, nCols, tiles):
        """Returns (packings: list[bytes|None], codec index used uint8 (255 = none), status)."""
        v = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, nRows * nCols)
        nt = v.shape[0]
        offsets = np.zeros(nt + 1, np.uint64)
        used = np.zeros(nt, np.uint8)
        status = np.zeros(nt, np.int32)
        fn = lib().gf_codec_master_encode_batch_i32
        st, blob = _grown_blob(lambda blob, cap: fn(self.ctx.handle, _ptr(self.codecs), self.codecs.size, nRows, nCols, nt, _ptr(v), _ptr(blob),
                                                    cap, _ptr(offsets), _ptr(used), _ptr(status)),
                               nt * (4 * nRows * nCols + 1024) + 64, 64, offsets)
        check(st, "gf_codec_master_encode_batch_i32")
        return _records_out(blob, offsets, nt, status), used, status

    def decode_batch(self, nRows, nCols, packings):
        nt = len(packings)
        blob, offsets = _blob_of(packings)
        out = np.zeros((nt, nRows * nCols), np.int32)
        status = np.zeros(nt, np.int32)
        _call("gf_codec_master_decode_batch_i32", self.ctx.handle, _ptr(self.codecs), self.codecs.size, nRows, nCols, nt, _ptr(blob),
              _ptr(offsets), _ptr(out), _ptr(status))
        return out, status

    # ---- tile payloads: RasterTile.getCompressedPacking over TileElementInt.encode (one integer element per tile) ----
    def tile_payloads(self, nRows, nCols, tiles):
        """Returns (payloads: list[bytes], codec index used uint8 (255 = raw cells))."""
        v = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, nRows * nCols)
        nt = v.shape[0]
        cap = nt * (4 * nRows * nCols + 8)
        blob = np.empty(cap, np.uint8)
        offsets = np.zeros(nt + 1, np.uint64)
        used = np.zeros(nt, np.uint8)
        _call("gf_tile_payload_encode_batch_i32", self.ctx.handle, _ptr(self.codecs), self.codecs.size, nRows, nCols, nt, _ptr(v), _ptr(blob),
              cap, _ptr(offsets), _ptr(used))
        return _records_out(blob, offsets, nt), used

    def tiles_from_payloads(self, nRows, nCols, payloads):
        nt = len(payloads)
        blob, offsets = _blob_of(payloads)
        out = np.zeros((nt, nRows * nCols), np.int32)
        status = np.zeros(nt, np.int32)
        _call("gf_tile_payload_decode_batch_i32", self.ctx.handle, _ptr(self.codecs), self.codecs.size, nRows, nCols, nt, _ptr(blob),
              _ptr(offsets), _ptr(out), _ptr(status))
        return out, status

    # ---- tile records: RecordManager.writeTile / readTile for a batch of dirty tiles (one integer-coded element) ----
    def tile_records(self, nRows, nCols, tile_indices, tiles, element="int", fill_value=-32768, checksums=True):
        """Returns (records: list[bytes] exactly as RecordManager appends them to the file, codec index used (255 = raw))."""
        short = element == "short"
        v = np.ascontiguousarray(tiles, dtype=np.int16 if short else np.int32).reshape(-1, nRows * nCols)
        nt = v.shape[0]
        idx = np.ascontiguousarray(tile_indices, dtype=np.int32)
        assert idx.size == nt
        cap = nt * int(lib().gf_tile_record_max_bytes(int(short), nRows, nCols))
        blob = np.empty(max(cap, 16), np.uint8)
        offsets = np.zeros(nt + 1, np.uint64)
        used = np.zeros(nt, np.uint8)
        _call("gf_tile_record_encode_batch", *self._head(), int(short), int(fill_value), nRows, nCols, nt, _ptr(idx), _ptr(v),
              int(bool(checksums)), _ptr(blob), cap, _ptr(offsets), _ptr(used))
        return _records_out(blob, offsets, nt), used

    def tiles_from_records(self, nRows, nCols, records, element="int", verify_checksums=True):
        """Returns (tile indices, values [nt, cells] int32 / int16, status per record)."""
        short = element == "short"
        nt = len(records)
        blob, offsets = _blob_of(records)
        out = np.zeros((nt, nRows * nCols), np.int16 if short else np.int32)
        idx = np.full(nt, -1, np.int32)
        status = np.zeros(nt, np.int32)
        _call("gf_tile_record_decode_batch", *self._head(), int(short), nRows, nCols, nt, _ptr(blob), _ptr(offsets), int(bool(verify_checksums)),
              _ptr(idx), _ptr(out), _ptr(status))
        return idx, out, status

    # ---- the same two readers for bytes in device memory: one upload of the bytes, everything else on the GPU ----
    def record_blob_dev(self, nRows, nCols, blob, offsets, element="int", verify_checksums=True):
        """gf_tile_record_decode_batch_dev on records as they lie in a byte array: record t = blob[offsets[t]:offsets[t+1]]
        (any byte alignment, anything between and behind the records).  Uploads blob and offsets, downloads the results:
        (tile indices, values [nt, cells] int32 / int16, status per record).  A caller whose bytes or consumer are on the
        device calls the entry point itself, with DeviceBuffer pointers."""
        short = element == "short"
        blob, offsets = _records_in(blob, offsets)
        nt, cells, dt = offsets.size - 1, nRows * nCols, np.dtype(np.int16 if short else np.int32)
        with _DeviceScope(self.ctx) as s:
            d_blob = s.upload(blob, slack=32, fill=0)
            d_off = s.upload(offsets)
            d_idx = s.alloc(nt * 4 + 16, fill=0xff)
            d_val = s.alloc(nt * cells * dt.itemsize + 16, fill=0)
            d_st = s.alloc(nt * 4 + 16, fill=0)
            s.run("gf_tile_record_decode_batch_dev", *self._head(stream=True), int(short), nRows, nCols, nt, d_blob.ptr, blob.size, d_off.ptr,
                  int(bool(verify_checksums)), d_idx.ptr, d_val.ptr, d_st.ptr)
            return d_idx.download(np.int32, nt), d_val.download(dt, nt * cells).reshape(nt, cells), d_st.download(np.int32, nt)

    def tiles_from_records_dev(self, nRows, nCols, records, element="int", verify_checksums=True):
        """tiles_from_records with the records decoded where they lie in device memory (gf_tile_record_decode_batch_dev)."""
        blob, offsets = _blob_of(records)
        blob = blob[:int(offsets[-1])]
        return self.record_blob_dev(nRows, nCols, blob, offsets, element=element, verify_checksums=verify_checksums)

    # ---- records of several elements, float and int-coded-float elements (gf_tile_record_decode_batch_elems[_dev]) ----
    @staticmethod
    def _elem_specs(elems):
        """elems: per element "int" | "short" | "float" | ("icf", scale, offset, fill_i, fill_f) -> (gf_elem_spec array, value dtypes)"""
        specs = np.zeros(len(elems), _ELEM_SPEC)
        dtypes = []
        for e, el in enumerate(elems):
            _, kind, params = _elem_kind(el)
            specs[e]["type"], specs[e]["scale"] = kind.type, 1.0
            if params is not None:
                specs[e]["scale"], specs[e]["offset"], specs[e]["fill_i"], specs[e]["fill_f"] = params
            dtypes.append(kind.delivered)
        return specs, dtypes

    def record_blob_elems_dev(self, nRows, nCols, blob, offsets, elems, verify_checksums=True):
        """gf_tile_record_decode_batch_elems_dev on records as they lie in a byte array (as record_blob_dev), for tiles of
        len(elems) elements (see _elem_specs).  Uploads blob and offsets, downloads the results: (tile indices, [values
        [nt, cells] per element: int32 / int16 / float32], status [n_elems, nt]).  A tile is good iff all its statuses are 0."""
        specs, dtypes = self._elem_specs(elems)
        blob, offsets = _records_in(blob, offsets)
        nt, ne, cells = offsets.size - 1, len(dtypes), nRows * nCols
        with _DeviceScope(self.ctx) as s:
            d_blob = s.upload(blob, slack=32, fill=0)
            d_off = s.upload(offsets)
            d_idx = s.alloc(nt * 4 + 16, fill=0xff)
            d_val = [s.alloc(nt * cells * np.dtype(dt).itemsize + 16, fill=0) for dt in dtypes]
            d_st = s.alloc(ne * nt * 4 + 16, fill=0)
            s.run("gf_tile_record_decode_batch_elems_dev", *self._head(stream=True), _ptr(specs), ne, nRows, nCols, nt, d_blob.ptr, blob.size,
                  d_off.ptr, int(bool(verify_checksums)), d_idx.ptr, s.ptrs(d_val), d_st.ptr)
            idx = d_idx.download(np.int32, nt)
            out = [b.download(dt, nt * cells).reshape(nt, cells) for b, dt in zip(d_val, dtypes)]
            return idx, out, d_st.download(np.int32, ne * nt).reshape(ne, nt)

    def record_blob_elems(self, nRows, nCols, blob, offsets, elems, verify_checksums=True):
        """The same through gf_tile_record_decode_batch_elems, the host-memory form (staged by the library, not pipelined);
        offsets[-1] bytes of blob are read."""
        specs, dtypes = self._elem_specs(elems)
        blob, offsets = _records_in(blob, offsets, tail=True)
        nt, ne, cells = offsets.size - 1, len(dtypes), nRows * nCols
        idx = np.full(nt, -1, np.int32)
        out = [np.zeros((nt, cells), dt) for dt in dtypes]
        status = np.zeros((ne, nt), np.int32)
        _call("gf_tile_record_decode_batch_elems", *self._head(), _ptr(specs), ne, nRows, nCols, nt, _ptr(blob), _ptr(offsets),
              int(bool(verify_checksums)), _ptr(idx), _ptrs(out), _ptr(status))
        return idx, out, status

    # ---- records of several elements written (gf_tile_record_encode_batch_elems[_dev]) ----
    @staticmethod
    def _elem_values(nRows, nCols, values_per_element, elems, fills):
        """(gf_elem_spec array, [values [nt, cells] per element in the type the call takes: int32 (int, icf codes) / int16 / float32 bits])"""
        specs, _ = CodecMasterHip._elem_specs(elems)
        vals = []
        for e, el in enumerate(elems):
            name, kind, _ = _elem_kind(el)
            vals.append(np.ascontiguousarray(values_per_element[e], dtype=kind.written).reshape(-1, nRows * nCols))
            if name == "short":
                specs[e]["fill_i"] = kind.fill[1] if fills is None or fills[e] is None else fills[e]
        assert len({v.shape[0] for v in vals}) == 1
        return specs, vals

    def tile_records_elems(self, nRows, nCols, tile_indices, values_per_element, elems, checksums=True, fills=None):
        """gf_tile_record_encode_batch_elems, the host-memory form, for tiles of len(elems) elements (see _elem_specs; an "icf"
        element's values are its int32 codes; fills: per "short" element its fill value, default -32768).  Returns (records:
        list[bytes] exactly as RecordManager appends them to the file, codec index used [n_elems, nt] (255 = standard form))."""
        specs, vals = self._elem_values(nRows, nCols, values_per_element, elems, fills)
        nt, ne = vals[0].shape[0], len(vals)
        idx = np.ascontiguousarray(tile_indices, dtype=np.int32)
        assert idx.size == nt
        cap = nt * int(lib().gf_tile_record_max_bytes_elems(_ptr(specs), ne, nRows, nCols))
        blob = np.empty(max(cap, 16), np.uint8)
        offsets = np.zeros(nt + 1, np.uint64)
        used = np.zeros((ne, nt), np.uint8)
        _call("gf_tile_record_encode_batch_elems", *self._head(), _ptr(specs), ne, nRows, nCols, nt, _ptr(idx), _ptrs(vals), int(bool(checksums)),
              _ptr(blob), cap, _ptr(offsets), _ptr(used))
        return _records_out(blob, offsets, nt), used

    def tile_records_elems_dev(self, nRows, nCols, tile_indices, values_per_element, elems, checksums=True, fills=None, blob_cap=None,
                               raw=False):
        """gf_tile_record_encode_batch_elems_dev: uploads the tiles, calls the device form, synchronises and downloads.  Returns
        (records, codec index used [n_elems, nt], status per tile); with raw=True (blob, offsets, used, status) instead of the list
        of records: the whole blob of blob_cap bytes (default: room for every record in standard form) pre-filled with 0xA5."""
        specs, vals = self._elem_values(nRows, nCols, values_per_element, elems, fills)
        nt, ne = vals[0].shape[0], len(vals)
        idx = np.ascontiguousarray(tile_indices, dtype=np.int32)
        assert idx.size == nt
        full = nt * int(lib().gf_tile_record_max_bytes_elems(_ptr(specs), ne, nRows, nCols))
        cap = full if blob_cap is None else int(blob_cap)
        with _DeviceScope(self.ctx) as s:
            d_val = [s.upload(v, slack=16) for v in vals]
            d_idx = s.upload(idx, slack=16)
            d_blob = s.alloc(max(cap, full) + 64, fill=0xA5)
            d_off = s.alloc((nt + 1) * 8 + 16, fill=0xff)
            d_used = s.alloc(ne * nt + 16, fill=0)
            d_st = s.alloc(nt * 4 + 16, fill=0x7f)
            s.run("gf_tile_record_encode_batch_elems_dev", *self._head(stream=True), _ptr(specs), ne, nRows, nCols, nt, d_idx.ptr, s.ptrs(d_val),
                  int(bool(checksums)), d_blob.ptr, cap, d_off.ptr, d_used.ptr, d_st.ptr)
            offsets = d_off.download(np.uint64, nt + 1)
            blob = d_blob.download(np.uint8, max(cap, full) + 64)
            used = d_used.download(np.uint8, ne * nt).reshape(ne, nt)
            status = d_st.download(np.int32, nt)
        if raw:
            return blob, offsets, used, status
        return _records_out(blob, offsets, nt), used, status

    # ---- grid blocks: GvrsElement.readBlock for a batch of records (gf_block_read_elems[_dev]) ----
    @staticmethod
    def _fill_specs(specs, elems, fills):
        """fills: per element None (INT4_NULL_CODE / -32768 / NaN) or the block's fill value; an ICF element's is its own fill_f"""
        for e, el in enumerate(elems):
            _, kind, _ = _elem_kind(el)
            f = None if fills is None else fills[e]
            if kind.fill is None:
                assert f is None, "an int-coded-float element is filled with the fill_f of its description"
            else:
                field, default = kind.fill
                specs[e][field] = default if f is None else f
        return specs

    def _read_args(self, nRows, nCols, grid_shape, rect, factor, blob, offsets, elems, fills, tail):
        """What the block readers share.  factor None: the block itself in the delivered dtypes; else the block downsampled by it, in
        the coarse dtypes.  -> (specs, dtypes, blob, offsets, grid, rect, the block's shape, (factor,) or ())"""
        specs, dtypes = self._elem_specs(elems)
        self._fill_specs(specs, elems, fills)
        blob, offsets = _records_in(blob, offsets, tail=tail)
        grid, rect = _grid_rect(nRows, nCols, grid_shape, rect)
        if factor is None:
            return specs, dtypes, blob, offsets, grid, rect, (int(rect[2]), int(rect[3])), ()
        shape = GvrsHipContext.downsample_rect(rect, factor)[2:]
        return specs, self._coarse_dtypes(elems, dtypes), blob, offsets, grid, rect, shape, (int(factor),)

    def _read_blocks_dev(self, name, nRows, nCols, grid_shape, rect, factor, blob, offsets, elems, fills, verify_checksums):
        specs, dtypes, blob, offsets, grid, rect, shape, factor = self._read_args(nRows, nCols, grid_shape, rect, factor, blob, offsets, elems,
                                                                                  fills, False)
        nt, ne, n_block = offsets.size - 1, len(dtypes), shape[0] * shape[1]
        with _DeviceScope(self.ctx) as s:
            d_blob = s.upload(blob, slack=32, fill=0)
            d_off = s.upload(offsets)
            d_blk = [s.alloc(n_block * np.dtype(dt).itemsize + 16, fill=0) for dt in dtypes]
            d_st = s.alloc(ne * nt * 4 + 16, fill=0)
            s.run(name, *self._head(stream=True), _ptr(specs), ne, _ptr(grid), _ptr(rect), *factor, nt, d_blob.ptr, blob.size, d_off.ptr,
                  int(bool(verify_checksums)), s.ptrs(d_blk), d_st.ptr)
            return [b.download(dt, n_block).reshape(shape) for b, dt in zip(d_blk, dtypes)], d_st.download(np.int32, ne * nt).reshape(ne, nt)

    def read_block_dev(self, nRows, nCols, grid_shape, rect, blob, offsets, elems, fills=None, verify_checksums=True):
        """gf_block_read_elems_dev: the rectangle rect = (row0, col0, n_rows, n_cols) of a grid of grid_shape = (rows, columns)
        cells cut into nRows x nCols tiles, read from tile records as they lie in a byte array (as record_blob_elems_dev; records
        in any order, tiles the bytes do not hold read as fill).  Uploads blob and offsets, downloads the results: ([block
        [n_rows, n_cols] per element: int32 / int16 / float32], status [n_elems, nt]).  The block is good iff every status is 0."""
        return self._read_blocks_dev("gf_block_read_elems_dev", nRows, nCols, grid_shape, rect, None, blob, offsets, elems, fills, verify_checksums)

    def read_block(self, nRows, nCols, grid_shape, rect, blob, offsets, elems, fills=None, verify_checksums=True):
        """The same through gf_block_read_elems, the host-memory form (staged by the library); offsets[-1] bytes of blob are read."""
        specs, dtypes, blob, offsets, grid, rect, shape, _ = self._read_args(nRows, nCols, grid_shape, rect, None, blob, offsets, elems, fills, True)
        nt, ne = offsets.size - 1, len(dtypes)
        out = [np.zeros(shape, dt) for dt in dtypes]
        status = np.zeros((ne, nt), np.int32)
        _call("gf_block_read_elems", *self._head(), _ptr(specs), ne, _ptr(grid), _ptr(rect), nt, _ptr(blob), _ptr(offsets),
              int(bool(verify_checksums)), _ptrs(out), _ptr(status))
        return out, status

    # ---- grid blocks read and downsampled: records in, one coarse block per element out (gf_block_read_downsampled_elems[_dev]) ----
    @staticmethod
    def _coarse_dtypes(elems, dtypes):
        """an int-coded-float element comes back as its int32 codes"""
        return [_elem_kind(el)[1].coarse for el in elems]

    def read_block_downsampled_dev(self, nRows, nCols, grid_shape, rect, factor, blob, offsets, elems, fills=None, verify_checksums=True):
        """gf_block_read_downsampled_elems_dev: read_block_dev's arguments plus factor.  Returns ([coarse block [n_rows', n_cols'] per
        element for downsample_rect(rect, factor): int32 / int16 / float32, an "icf" element as int32 codes], status [n_elems, nt]);
        the blocks are good iff every status is 0."""
        return self._read_blocks_dev("gf_block_read_downsampled_elems_dev", nRows, nCols, grid_shape, rect, factor, blob, offsets, elems, fills,
                                     verify_checksums)

    def read_block_downsampled(self, nRows, nCols, grid_shape, rect, factor, blob, offsets, elems, fills=None, verify_checksums=True):
        """The same through gf_block_read_downsampled_elems, the host-memory form; offsets[-1] bytes of blob are read."""
        specs, dtypes, blob, offsets, grid, rect, (n_rows, n_cols), factor = self._read_args(nRows, nCols, grid_shape, rect, factor, blob, offsets,
                                                                                             elems, fills, True)
        nt, ne = offsets.size - 1, len(dtypes)
        out = [np.zeros(max(n_rows * n_cols, 1), dt) for dt in dtypes]
        status = np.zeros((ne, nt), np.int32)
        _call("gf_block_read_downsampled_elems", *self._head(), _ptr(specs), ne, _ptr(grid), _ptr(rect), *factor, nt, _ptr(blob), _ptr(offsets),
              int(bool(verify_checksums)), _ptrs(out), _ptr(status))
        return [a[:n_rows * n_cols].reshape(n_rows, n_cols) for a in out], status

    # ---- a rectangle read from tile records and its symbols counted onto a table (gf_block_read_tabulated_symbols_elems[_dev]) ----
    def read_block_tabulated_symbols_dev(self, nRows, nCols, grid_shape, rect, blob, offsets, elems, which, into=None, fills=None,
                                         verify_checksums=True, table_cap=None):
        """gf_block_read_tabulated_symbols_elems_dev: read_block_dev's arguments, the element `which` whose symbols are counted (an
        "icf" element as its int32 codes) and the table into = (symbols, counts, summary dict) they are counted onto (None: empty).
        Uploads and downloads: ((symbols, counts, summary dict), status [n_elems, nt]); good iff every status is 0."""
        specs, dtypes, blob, offsets, grid, rect, shape, _ = self._read_args(nRows, nCols, grid_shape, rect, None, blob, offsets, elems, fills, False)
        nt, ne = offsets.size - 1, len(dtypes)
        sym_in, cnt_in, sum_in, _ = _tab_table_in(into)
        n_in = 0 if into is None else sym_in.size
        cap = n_in + shape[0] * shape[1] if table_cap is None else int(table_cap)
        with _DeviceScope(self.ctx) as s:
            d_blob, d_off = s.upload(blob, slack=32, fill=0), s.upload(offsets)
            d_in = [s.upload(a, slack=16) for a in (sym_in, cnt_in, sum_in)] if into is not None else None
            d_sym, d_cnt, d_sum = s.alloc(cap * 4 + 16, fill=0), s.alloc(cap * 4 + 16, fill=0), s.alloc(TAB_SYMBOLS.itemsize, fill=0)
            d_st = s.alloc(ne * nt * 4 + 16, fill=0)
            in_args = (None, None, None, 0) if d_in is None else (d_in[0].ptr, d_in[1].ptr, d_in[2].ptr, n_in)
            s.run("gf_block_read_tabulated_symbols_elems_dev", *self._head(), _ptr(specs), ne, _ptr(grid), _ptr(rect), nt, d_blob.ptr, blob.size,
                  d_off.ptr, int(bool(verify_checksums)), int(which), *in_args, d_sym.ptr if cap else None, d_cnt.ptr if cap else None, cap,
                  d_sum.ptr, d_st.ptr)
            summary = d_sum.download(TAB_SYMBOLS, 1)
            n = int(summary["n_written"][0])
            table = (d_sym.download(np.uint32, n), d_cnt.download(np.int32, n), {k: summary[k][0].item() for k in TAB_SYMBOLS.names})
            return table, d_st.download(np.int32, ne * nt).reshape(ne, nt)

    def read_block_tabulated_symbols(self, nRows, nCols, grid_shape, rect, blob, offsets, elems, which, into=None, fills=None,
                                     verify_checksums=True, table_cap=None):
        """The same through gf_block_read_tabulated_symbols_elems, the host-memory form; offsets[-1] bytes of blob are read."""
        specs, dtypes, blob, offsets, grid, rect, shape, _ = self._read_args(nRows, nCols, grid_shape, rect, None, blob, offsets, elems, fills, True)
        nt, ne = offsets.size - 1, len(dtypes)
        si, ci, ui, arg_in = _tab_table_in(into)
        cap = arg_in[3] + shape[0] * shape[1] if table_cap is None else int(table_cap)
        status = np.zeros((ne, nt), np.int32)
        fn = lib().gf_block_read_tabulated_symbols_elems
        table = _tab_table_out("gf_block_read_tabulated_symbols_elems", cap,
                               lambda sym, cnt, n, summ: fn(*self._head(), _ptr(specs), ne, _ptr(grid), _ptr(rect), nt, _ptr(blob), _ptr(offsets),
                                                            int(bool(verify_checksums)), int(which), *arg_in, sym, cnt, n, summ, _ptr(status)))
        return table, status

    # ---- grid blocks written: raster in, tile records out (gf_block_write_elems[_dev]) ----
    @staticmethod
    def _range_specs(specs, elems, ranges):
        """ranges: None (the library's defaults: NULL is passed) or per element None | (min, max) -> gf_elem_range array or None"""
        if ranges is None:
            return None
        out = np.zeros(len(elems), _ELEM_RANGE)
        for e, el in enumerate(elems):
            name, kind, _ = _elem_kind(el)
            suffix, lo, hi = kind.range
            if name == "icf":                  # the codes' range as values
                scale, offset = np.float32(specs[e]["scale"]), np.float32(specs[e]["offset"])
                lo, hi = np.float32(lo) / scale + offset, np.float32(hi) / scale + offset
            out[e]["min_" + suffix], out[e]["max_" + suffix] = (lo, hi) if ranges[e] is None else ranges[e]
        return out

    def _write_dev(self, name, head, source, n_elems, n_out, full, old, checksums, verify_old_checksums, blob_cap, raw):
        """What write_block_dev and image_write_dev share: source (the arrays uploaded first, by the function that turns their buffers
        into the call's arguments behind head), the old records, the output buffers, the call and what comes back."""
        arrays, source_args = source
        old_blob, old_off, n_old = _old_records(old)
        cap = full if blob_cap is None else int(blob_cap)
        with _DeviceScope(self.ctx) as s:
            d_src = [s.upload(a, slack=16) for a in arrays]
            d_oblob = s.upload(old_blob, slack=32, fill=0)
            d_ooff = s.upload(old_off, slack=16)
            d_blob = s.alloc(max(cap, full) + 64, fill=0xA5)
            d_off = s.alloc((n_out + 1) * 8 + 16, fill=0xff)
            d_idx = s.alloc(n_out * 4 + 16, fill=0x7f)
            d_used = s.alloc(n_elems * n_out + 16, fill=0)
            d_st = s.alloc(n_out * 4 + 16, fill=0x7f)
            s.run(name, *head, source_args(d_src), n_old, d_oblob.ptr if n_old else None, int(old_off[-1]) if n_old else 0,
                  d_ooff.ptr if n_old else None, int(bool(verify_old_checksums)), int(bool(checksums)), d_blob.ptr, cap, d_off.ptr, d_idx.ptr,
                  d_used.ptr, d_st.ptr)
            offsets = d_off.download(np.uint64, n_out + 1)
            blob = d_blob.download(np.uint8, max(cap, full) + 64)
            idx = d_idx.download(np.int32, n_out)
            used = d_used.download(np.uint8, n_elems * n_out).reshape(n_elems, n_out)
            status = d_st.download(np.int32, n_out)
        if raw:
            return idx, blob, offsets, used, status
        return idx, _records_out(blob, offsets, n_out), used, status

    def _write_host(self, name, head, source, n_elems, n_out, full, old, checksums, verify_old_checksums, blob_cap, checked=True):
        """The same for write_block and image_write, the host forms -> (the call's return value, checked unless told otherwise; tile
        indices, blob, offsets, codec used, status, the blob's capacity)"""
        old_blob, old_off, n_old = _old_records(old)
        old_blob, old_off = _records_in(old_blob, old_off, tail=True)
        cap = full if blob_cap is None else int(blob_cap)
        blob = np.empty(max(cap, 16), np.uint8)
        offsets = np.zeros(n_out + 1, np.uint64)
        idx = np.full(n_out, -1, np.int32)
        used = np.zeros((n_elems, n_out), np.uint8)
        status = np.full(n_out, 0x7f7f7f7f, np.int32)
        rc = getattr(lib(), name)(*head, source, n_old, _ptr(old_blob) if n_old else None, _ptr(old_off) if n_old else None,
                                  int(bool(verify_old_checksums)), int(bool(checksums)), _ptr(blob), cap, _ptr(offsets), _ptr(idx), _ptr(used),
                                  _ptr(status))
        if checked:
            check(rc, name)
        return rc, idx, blob, offsets, used, status, cap

    def _block_write_args(self, nRows, nCols, grid_shape, rect, blocks, elems, fills, ranges):
        """-> (the call's arguments from the element specs to rect; the arrays they point into, which the caller holds until the call is
        over; the blocks flat in their dtypes; the number of tiles written; room for every record in standard form)"""
        specs, dtypes = self._elem_specs(elems)
        self._fill_specs(specs, elems, fills)
        rng = self._range_specs(specs, elems, ranges)
        grid, rect = _grid_rect(nRows, nCols, grid_shape, rect)
        n_block = int(rect[2]) * int(rect[3])
        blocks = [np.ascontiguousarray(b, dtype=dt).reshape(-1) for b, dt in zip(blocks, dtypes)]
        assert len(blocks) == len(dtypes) and all(b.size == n_block for b in blocks)
        n_out = _tiles_of_rect(grid, rect)
        full = n_out * int(lib().gf_tile_record_max_bytes_elems(_ptr(specs), len(dtypes), nRows, nCols))
        return (_ptr(specs), None if rng is None else _ptr(rng), len(blocks), _ptr(grid), _ptr(rect)), (specs, rng, grid, rect), blocks, n_out, full

    def write_block_dev(self, nRows, nCols, grid_shape, rect, blocks, elems, fills=None, ranges=None, old=None, checksums=True,
                        verify_old_checksums=True, blob_cap=None, raw=False):
        """gf_block_write_elems_dev: the rectangle rect = (row0, col0, n_rows, n_cols) of a grid of grid_shape cells cut into nRows x
        nCols tiles is written from blocks (per element [n_rows, n_cols]: int32 / int16 / float32, an "icf" element's float VALUES)
        as tile records.  fills as read_block_dev; ranges: None or per element None | (min, max); old = (blob, offsets): records the
        file already holds, merged into partly covered tiles.  Uploads, calls, synchronises, downloads: (tile indices [n_out],
        records: list[bytes], b"" for a tile without one, codec used [n_elems, n_out], status [n_out]); raw=True: (tile indices,
        blob, offsets, codec used, status) with the whole blob of blob_cap bytes + 64 pre-filled with 0xA5."""
        args, _held, blocks, n_out, full = self._block_write_args(nRows, nCols, grid_shape, rect, blocks, elems, fills, ranges)
        return self._write_dev("gf_block_write_elems_dev", self._head(stream=True) + args, (blocks, _ptrs), len(blocks), n_out, full, old,
                               checksums, verify_old_checksums, blob_cap, raw)

    def write_block(self, nRows, nCols, grid_shape, rect, blocks, elems, fills=None, ranges=None, old=None, checksums=True,
                    verify_old_checksums=True, blob_cap=None, return_code=False):
        """The same through gf_block_write_elems, the host-memory form, which takes any codec list.  Returns (tile indices, records,
        codec used, status); a negative per-tile status or too small a blob_cap raises as the library returns it, unless
        return_code is set: then (the call's return value, tile indices, records, codec used, status, offsets) come back."""
        args, _held, blocks, n_out, full = self._block_write_args(nRows, nCols, grid_shape, rect, blocks, elems, fills, ranges)
        rc, idx, blob, offsets, used, status, cap = self._write_host("gf_block_write_elems", self._head() + args, _ptrs(blocks), len(blocks), n_out,
                                                                     full, old, checksums, verify_old_checksums, blob_cap,
                                                                     checked=not return_code)
        if return_code:
            fits = int(offsets[-1]) <= cap
            return rc, idx, (_records_out(blob, offsets, n_out) if fits else [None] * n_out), used, status, offsets
        return idx, _records_out(blob, offsets, n_out), used, status

    # ---- ARGB images stored as tile records of three elements and read back (gf_image_write[_dev], gf_image_read[_dev]) ----
    def _image_args(self, nRows, nCols, grid_shape, rect, model, elem_type, fill):
        model, et, _ = GvrsHipContext._image_kind(model, elem_type)
        fill = _ELEM_KINDS["int" if et == ELEM_TYPES["int"] else "short"].fill[1] if fill is None else int(fill)
        specs = np.zeros(3, _ELEM_SPEC)
        specs["type"], specs["fill_i"] = et, fill
        grid, rect = _grid_rect(nRows, nCols, grid_shape, rect)
        n_out = _tiles_of_rect(grid, rect)
        full = n_out * int(lib().gf_tile_record_max_bytes_elems(_ptr(specs), 3, nRows, nCols))
        return model, et, fill, grid, rect, n_out, full

    @staticmethod
    def _image_words(argb, rect):
        a = _argb_words(argb)
        assert a.size == int(rect[2]) * int(rect[3])
        return a.reshape(-1)

    def image_write_dev(self, nRows, nCols, grid_shape, rect, argb, model="ycocg", elem_type="short", fill=None, old=None, checksums=True,
                        verify_old_checksums=True, blob_cap=None, raw=False):
        """gf_image_write_dev: rect's pixels (argb [n_rows, n_cols] words) stored as tile records of three elements -- the planes r,
        g, b ("rgb") or Y, Co, Cg ("ycocg") as "int" or "short" elements with fill `fill` -- as write_block_dev stores blocks, and
        returning what it returns.  Uploads, calls, synchronises, downloads."""
        model, et, fill, grid, rect, n_out, full = self._image_args(nRows, nCols, grid_shape, rect, model, elem_type, fill)
        argb = self._image_words(argb, rect)
        return self._write_dev("gf_image_write_dev", self._head() + (model, et, fill, _ptr(grid), _ptr(rect)), ([argb], lambda d: d[0].ptr), 3,
                               n_out, full, old, checksums, verify_old_checksums, blob_cap, raw)

    def image_write(self, nRows, nCols, grid_shape, rect, argb, model="ycocg", elem_type="short", fill=None, old=None, checksums=True,
                    verify_old_checksums=True, blob_cap=None):
        """The same through gf_image_write, the host-memory form, which takes any codec list: (tile indices, records, codec used,
        status); a negative per-tile status or too small a blob_cap raises."""
        model, et, fill, grid, rect, n_out, full = self._image_args(nRows, nCols, grid_shape, rect, model, elem_type, fill)
        argb = self._image_words(argb, rect)
        _, idx, blob, offsets, used, status, _ = self._write_host("gf_image_write", self._head() + (model, et, fill, _ptr(grid), _ptr(rect)),
                                                                   _ptr(argb), 3, n_out, full, old, checksums, verify_old_checksums, blob_cap)
        return idx, _records_out(blob, offsets, n_out), used, status

    def image_read_dev(self, nRows, nCols, grid_shape, rect, blob, offsets, model="ycocg", elem_type="short", fill=None, verify_checksums=True):
        """gf_image_read_dev: rect's pixels read from tile records of three elements as image_write_dev writes them: (argb [n_rows,
        n_cols] int32, status [3, n_records]).  The pixels of tiles the bytes do not hold are the join of three fills."""
        model, et, fill, grid, rect, _, _ = self._image_args(nRows, nCols, grid_shape, rect, model, elem_type, fill)
        blob, offsets = _records_in(blob, offsets)
        nt, n_px = offsets.size - 1, int(rect[2]) * int(rect[3])
        with _DeviceScope(self.ctx) as s:
            d_blob = s.upload(blob, slack=32, fill=0)
            d_off = s.upload(offsets)
            d_argb = s.alloc(n_px * 4 + 16, fill=0)
            d_st = s.alloc(3 * nt * 4 + 16, fill=0)
            s.run("gf_image_read_dev", *self._head(), model, et, fill, _ptr(grid), _ptr(rect), nt, d_blob.ptr, blob.size, d_off.ptr,
                  int(bool(verify_checksums)), d_argb.ptr, d_st.ptr)
            return d_argb.download(np.int32, n_px).reshape(int(rect[2]), int(rect[3])), d_st.download(np.int32, 3 * nt).reshape(3, nt)

    def image_read(self, nRows, nCols, grid_shape, rect, blob, offsets, model="ycocg", elem_type="short", fill=None, verify_checksums=True):
        """The same through gf_image_read, the host-memory form; offsets[-1] bytes of blob are read."""
        model, et, fill, grid, rect, _, _ = self._image_args(nRows, nCols, grid_shape, rect, model, elem_type, fill)
        blob, offsets = _records_in(blob, offsets, tail=True)
        nt = offsets.size - 1
        argb = np.zeros((int(rect[2]), int(rect[3])), np.int32)
        status = np.zeros((3, nt), np.int32)
        _call("gf_image_read", *self._head(), model, et, fill, _ptr(grid), _ptr(rect), nt, _ptr(blob), _ptr(offsets), int(bool(verify_checksums)),
              _ptr(argb), _ptr(status))
        return argb, status

    # ---- packings in device memory (gf_codec_master_decode_batch_i32_dev) ----
    def packing_blob_dev(self, nRows, nCols, blob, offsets, lengths):
        """gf_codec_master_decode_batch_i32_dev: packing t = blob[offsets[t]:offsets[t]+lengths[t]].  Returns (values, status)."""
        blob, offsets = _records_in(blob, offsets)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        nt = lengths.size
        assert offsets.size == nt
        cells = nRows * nCols
        with _DeviceScope(self.ctx) as s:
            d_blob = s.upload(blob, slack=32, fill=0)
            d_off = s.upload(offsets, slack=16)
            d_len = s.upload(lengths, slack=16)
            d_val = s.alloc(nt * cells * 4 + 16, fill=0)
            d_st = s.alloc(nt * 4 + 16, fill=0)
            s.run("gf_codec_master_decode_batch_i32_dev", *self._head(stream=True), nRows, nCols, nt, d_blob.ptr, blob.size, d_off.ptr, d_len.ptr,
                  d_val.ptr, d_st.ptr)
            return d_val.download(np.int32, nt * cells).reshape(nt, cells), d_st.download(np.int32, nt)

    def decode_batch_dev(self, nRows, nCols, packings):
        """decode_batch with the packings decoded where they lie in device memory (gf_codec_master_decode_batch_i32_dev)."""
        lengths = np.array([len(p) for p in packings], np.uint32)
        blob, offsets = _blob_of(packings)
        return self.packing_blob_dev(nRows, nCols, blob[:int(offsets[-1])], offsets[:-1], lengths)


# ---- GVRS files ----
class GvrsFileFacts:
    """What a file is written from (gf_file_facts, gf_file_metadata), held together with every buffer the structs point into.
    grid = (rows, columns of the grid, rows, columns of a tile); elems as the record calls take them ("int" | "short" | "float" |
    ("icf", scale, offset, fill_i, fill_f)), fills as read_block_dev; elem_facts: None (elements "e0", "e1", ... with the default
    ranges) or per element a dict of name, label, description, unit, continuous and range -- None, (min, max), or for an "icf"
    element (min_f, max_f, min_i, max_i); codec_ids: the specification's strings; bounds = (x0, y0, x1, y1), default the grid's
    cell indices; metadata: (name, record id, type code, content bytes, description) per record, laid in this order."""

    def __init__(self, grid, elems, fills=None, elem_facts=None, codec_ids=(), checksums=True, raster_space=0, coordinate_system=0, bounds=None,
                 cell_size=(1.0, 1.0), m2r=(1.0, 0.0, -0.0, 0.0, 1.0, -0.0), r2m=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0), product_label="", uuid=bytes(16),
                 time_modified=0, metadata=()):
        self.grid, self.elems = tuple(int(x) for x in grid), list(elems)
        self._held = []
        self.specs, self.dtypes = CodecMasterHip._elem_specs(self.elems)
        CodecMasterHip._fill_specs(self.specs, self.elems, fills)
        self._written = [_elem_kind(el)[1].delivered for el in self.elems]
        f = np.zeros(1, _FILE_FACTS)
        f["grid"], f["n_elems"], f["n_codecs"] = self.grid, len(self.elems), len(codec_ids)
        f["elems"] = self.specs.ctypes.data
        if elem_facts is not None:
            assert len(elem_facts) == len(self.elems)
            x = np.zeros(len(self.elems), _FILE_ELEM_FACTS)
            for e, d in enumerate(elem_facts):
                for k in ("name", "label", "description", "unit"):
                    x[e][k] = self._str(d.get(k))
                x[e]["continuous"] = int(bool(d.get("continuous", False)))
                r = d.get("range")
                if r is not None:
                    kind = _elem_kind(self.elems[e])[0]
                    x[e]["has_range"] = 1
                    if kind == "icf":
                        x[e]["range"]["min_f"], x[e]["range"]["max_f"], x[e]["range"]["min_i"], x[e]["range"]["max_i"] = r
                    else:
                        suffix = _ELEM_KINDS[kind].range[0]
                        x[e]["range"]["min_" + suffix], x[e]["range"]["max_" + suffix] = r
            self._held.append(x)
            f["elem_facts"] = x.ctypes.data
        ids = (C.c_char_p * max(len(codec_ids), 1))(*[c.encode() for c in codec_ids])
        self._held.append(ids)
        f["codec_ids"] = C.addressof(ids)
        f["product_label"] = self._str(product_label)
        f["checksum_enabled"], f["raster_space"], f["coordinate_system"] = int(bool(checksums)), raster_space, coordinate_system
        f["x0"], f["y0"], f["x1"], f["y1"] = (0.0, 0.0, float(self.grid[1] - 1), float(self.grid[0] - 1)) if bounds is None else bounds
        f["cell_size_x"], f["cell_size_y"] = cell_size
        f["m2r"], f["r2m"] = m2r, r2m
        f["uuid"] = np.frombuffer(bytes(uuid), np.uint8)
        f["time_modified"] = time_modified
        self.facts, self.checksums = f, bool(checksums)
        m = np.zeros(max(len(metadata), 1), _FILE_METADATA)
        for k, (name, record_id, type_code, content, description) in enumerate(metadata):
            content = np.frombuffer(bytes(content), np.uint8)
            self._held.append(content)
            m[k]["name"], m[k]["description"] = self._str(name), self._str(description)
            m[k]["content"], m[k]["content_bytes"] = (content.ctypes.data if content.size else 0), content.size
            m[k]["record_id"], m[k]["type"] = record_id, type_code
        self.metadata, self.n_metadata = m, len(metadata)

    def _str(self, s):
        """The address of a held 0-terminated copy of s; 0 (NULL) for None"""
        if s is None:
            return 0
        b = C.create_string_buffer(s if isinstance(s, bytes) else s.encode())
        self._held.append(b)
        return C.addressof(b)

    def args(self):
        """(facts, metadata, n_metadata) as the entry points take them"""
        return _ptr(self.facts), (_ptr(self.metadata) if self.n_metadata else None), self.n_metadata

    def rect_args(self, rect):
        """-> (rect array, number of tiles it touches); None: the whole grid"""
        grid, rect = _grid_rect(self.grid[2], self.grid[3], self.grid[:2], (0, 0, self.grid[0], self.grid[1]) if rect is None else rect)
        return rect, _tiles_of_rect(grid, rect)

    def blocks_in(self, rect, blocks):
        n_block = int(rect[2]) * int(rect[3])
        blocks = [np.ascontiguousarray(b, dtype=dt).reshape(-1) for b, dt in zip(blocks, self._written)]
        assert len(blocks) == len(self.elems) and all(b.size == n_block for b in blocks)
        return blocks

    def plan(self, rect=None, flags=0):
        """gf_file_write_plan: (the first tile record's position, the largest image the rectangle can need)"""
        r = None if rect is None else self.rect_args(rect)[0]
        first, most = C.c_uint64(), C.c_uint64()
        _call("gf_file_write_plan", *self.args(), None if r is None else _ptr(r), int(flags), C.byref(first), C.byref(most))
        return first.value, most.value


class GvrsFileHip:
    """org.gridfour.gvrs.GvrsFile(file, "r") with GvrsElement.readBlock for all elements: a version 1.04 file opened from its path
    or its bytes (gf_file_open: the header record and the tile directory's prefix, parsed on the host), blocks read from the file
    image by gf_file_read_block_elems[_dev], cells and interpolated values at scattered points by gf_file_read_points_elems[_dev] and
    gf_file_interp_points[_dev] (only the tiles the points touch are decoded), the same at longitude / latitude or model x / y by
    map_points[_dev], read_coords and interp_coords[_dev]; and, as static methods, new file images written: assemble (tile records in, host
    memory), write_image (blocks in device memory in, the image out) and write_image_host; an image updated in place by
    update_image[_host] (a rectangle) and update_points[_host] (scattered cells: only the touched tiles are rewritten).  .info is the gf_file_info as a dict, with the elements' names, the codec ids and the
    product label; .elems are the elements as the record calls of CodecMasterHip take them."""

    _ELEM_NAMES = {kind.type: name for name, kind in _ELEM_KINDS.items()}

    def __init__(self, path_or_bytes):
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview, np.ndarray)):
            self.image = np.frombuffer(bytes(path_or_bytes), np.uint8)
        else:
            self.image = np.fromfile(path_or_bytes, np.uint8)
        self._h = C.c_void_p()
        _call("gf_file_open", _ptr(self.image), self.image.size, C.byref(self._h))
        raw = np.zeros(1, _FILE_INFO)
        _call("gf_file_get_info", self._h, _ptr(raw))
        raw = raw[0]
        L = lib()
        self.n_elems, self.grid = int(raw["n_elems"]), tuple(int(x) for x in raw["grid"])
        self._dtypes = [_delivered_dtype(raw["elems"][e]["type"]) for e in range(self.n_elems)]
        self.elems = []
        for e in range(self.n_elems):
            el = raw["elems"][e]
            name = self._ELEM_NAMES[int(el["type"])]
            self.elems.append(name if name != "icf" else ("icf", float(el["scale"]), float(el["offset"]), int(el["fill_i"]), float(el["fill_f"])))
        self.info = {k: (raw[k].tolist() if raw[k].ndim else raw[k].item()) for k in _FILE_INFO.names if k not in ("elems", "codecs", "grid")}
        self.info["grid"] = self.grid
        self.info["elems"] = [{k: raw["elems"][e][k].item() for k in _ELEM_SPEC.names} for e in range(self.n_elems)]
        self.info["codecs"] = [int(k) for k in raw["codecs"][:int(raw["n_codecs"])]]
        self.info["elem_names"] = [L.gf_file_elem_name(self._h, e).decode() for e in range(self.n_elems)]
        self.info["codec_ids"] = [L.gf_file_codec_id(self._h, k).decode() for k in range(int(raw["n_codecs"]))]
        self.info["product_label"] = L.gf_file_product_label(self._h).decode()

    def tile_position(self, tile_index, image=None):
        """gf_file_tile_position: the file position of the tile's record content, 0 for a tile the file does not hold; raises
        GvrsHipError where the directory's entry or the record head is refused.  image: other bytes than the file's own."""
        image = self.image if image is None else np.frombuffer(bytes(image), np.uint8)
        pos = C.c_uint64()
        _call("gf_file_tile_position", self._h, _ptr(image), image.size, int(tile_index), C.byref(pos))
        return pos.value

    def _read_args(self, rect, image):
        image = self.image if image is None else np.frombuffer(bytes(image), np.uint8)
        grid, rect = _grid_rect(self.grid[2], self.grid[3], self.grid[:2], rect)
        nt = _tiles_of_rect(grid, rect)
        return image, rect, nt, (int(rect[2]), int(rect[3]))

    def read_block_dev(self, ctx, rect, verify_checksums=True, image=None):
        """gf_file_read_block_elems_dev: rect = (row0, col0, n_rows, n_cols) of the grid read from the file image in device memory
        (uploaded here; image: other bytes than the file's own, for a file that changed behind its header).  Returns ([block
        [n_rows, n_cols] per element], status [n_elems, T], present [T]) over the T tiles the rectangle touches."""
        image, rect, nt, shape = self._read_args(rect, image)
        n_block = shape[0] * shape[1]
        with _DeviceScope(ctx) as s:
            d_image = s.upload(image, slack=32, fill=0)
            d_blk = [s.alloc(n_block * np.dtype(dt).itemsize + 16, fill=0) for dt in self._dtypes]
            d_st = s.alloc(self.n_elems * nt * 4 + 16, fill=0x7f)
            d_pr = s.alloc(nt + 16, fill=0x7f)
            s.run("gf_file_read_block_elems_dev", ctx.handle, self._h, d_image.ptr, image.size, _ptr(rect), int(bool(verify_checksums)),
                  s.ptrs(d_blk), d_st.ptr, d_pr.ptr)
            return ([b.download(dt, n_block).reshape(shape) for b, dt in zip(d_blk, self._dtypes)],
                    d_st.download(np.int32, self.n_elems * nt).reshape(self.n_elems, nt), d_pr.download(np.uint8, nt))

    def read_block(self, ctx, rect, verify_checksums=True, image=None):
        """The same through gf_file_read_block_elems, the host-memory form: only the records of the rectangle's tiles are staged."""
        image, rect, nt, shape = self._read_args(rect, image)
        out = [np.zeros(shape, dt) for dt in self._dtypes]
        status = np.full((self.n_elems, nt), 0x7f7f7f7f, np.int32)
        present = np.full(nt, 0x7f, np.uint8)
        _call("gf_file_read_block_elems", ctx.handle, self._h, _ptr(image), image.size, _ptr(rect), int(bool(verify_checksums)), _ptrs(out),
              _ptr(status), _ptr(present))
        return out, status, present

    # ---- reads at points (gf_file_cells_tiles, gf_file_interp_tiles, gf_file_read_points_elems[_dev], gf_file_interp_points[_dev]) ----
    def points_spec(self, elem=0, **kw):
        """interp_spec() for element elem of this file over its whole grid: wrap, target, row_spacing, col_spacing, row_fringe and
        col_fringe as there.  The point reads take grid, type and fill from the file; the block route reads them from the spec."""
        el = self.info["elems"][elem]
        return interp_spec(self.grid[0], self.grid[1], elem_type=el["type"], fill_i=el["fill_i"], **kw)

    def _touched(self, name, head, rows, cols):
        n = C.c_size_t()
        _call(name, *head, rows.size, _ptr(rows), _ptr(cols), None, 0, C.byref(n))
        tiles = np.zeros(n.value, np.int32)
        _call(name, *head, rows.size, _ptr(rows), _ptr(cols), _ptr(tiles) if tiles.size else None, tiles.size, C.byref(n))
        return tiles

    def cells_tiles(self, rows, cols):
        """gf_file_cells_tiles: the distinct tiles the cells (rows[i], cols[i]) touch, ascending; a cell outside the grid touches none."""
        rows, cols = np.ascontiguousarray(rows, np.int32).ravel(), np.ascontiguousarray(cols, np.int32).ravel()
        assert rows.size == cols.size
        return self._touched("gf_file_cells_tiles", (self._h,), rows, cols)

    def interp_tiles(self, spec, rows, cols):
        """gf_file_interp_tiles: the distinct tiles the 4 x 4 windows of the query points touch, ascending (spec: wrap and fringes)."""
        rows, cols = np.ascontiguousarray(rows, np.float64).ravel(), np.ascontiguousarray(cols, np.float64).ravel()
        assert rows.size == cols.size
        return self._touched("gf_file_interp_tiles", (self._h, _ptr(spec)), rows, cols)

    @staticmethod
    def _points_done(name, st, return_code):
        if st != _lib.ERR_CAPACITY or not return_code:
            check(st, name)

    def read_points_dev(self, ctx, rows, cols, verify_checksums=True, image=None, max_tiles=None, return_code=False):
        """gf_file_read_points_elems_dev: the cells (rows[i], cols[i]) of every element read from the file image in device memory
        (uploaded here), decoding only the tiles they touch.  max_tiles: the pool's room in tiles (default: the host's count).
        Returns ([values [n] per element], status [n_elems, n], the touched tiles' count); return_code: ERR_CAPACITY does not
        raise and (..., the call's status, the 16 bytes behind every output buffer) is returned, the outputs as they were pre-set
        (every byte 0x7f) where the call wrote nothing."""
        image = self.image if image is None else np.frombuffer(bytes(image), np.uint8)
        rows, cols = np.ascontiguousarray(rows, np.int32).ravel(), np.ascontiguousarray(cols, np.int32).ravel()
        assert rows.size == cols.size
        n = rows.size
        max_tiles = self.cells_tiles(rows, cols).size if max_tiles is None else int(max_tiles)
        touched = C.c_size_t()
        with _DeviceScope(ctx) as s:
            d_image = s.upload(image, slack=32, fill=0)
            d_rows, d_cols = s.upload(rows, slack=16), s.upload(cols, slack=16)
            d_val = [s.alloc(n * np.dtype(dt).itemsize + 16, fill=0x7f) for dt in self._dtypes]
            d_st = s.alloc(self.n_elems * n * 4 + 16, fill=0x7f)
            st = lib().gf_file_read_points_elems_dev(ctx.handle, self._h, d_image.ptr, image.size, n, d_rows.ptr, d_cols.ptr,
                                                     int(bool(verify_checksums)), max_tiles, s.ptrs(d_val), d_st.ptr, C.byref(touched))
            self._points_done("gf_file_read_points_elems_dev", st, return_code)
            ctx.synchronize()
            out = ([b.download(dt, n) for b, dt in zip(d_val, self._dtypes)], d_st.download(np.int32, self.n_elems * n).reshape(self.n_elems, n),
                   touched.value)
            if not return_code:
                return out
            slack = [b.download(np.uint8, 16, n * np.dtype(dt).itemsize) for b, dt in zip(d_val, self._dtypes)]
            return out + (st, slack + [d_st.download(np.uint8, 16, self.n_elems * n * 4)])

    def read_points(self, ctx, rows, cols, verify_checksums=True, image=None, max_tiles=None, return_code=False):
        """The same through gf_file_read_points_elems, the host-memory form: only the touched tiles' records are staged.
        return_code: (..., the call's status)."""
        image = self.image if image is None else np.frombuffer(bytes(image), np.uint8)
        rows, cols = np.ascontiguousarray(rows, np.int32).ravel(), np.ascontiguousarray(cols, np.int32).ravel()
        assert rows.size == cols.size
        n = rows.size
        max_tiles = self.cells_tiles(rows, cols).size if max_tiles is None else int(max_tiles)
        out = [np.full(n, 0x7f, np.uint8).repeat(np.dtype(dt).itemsize).view(dt) for dt in self._dtypes]
        status = np.full((self.n_elems, n), 0x7f7f7f7f, np.int32)
        touched = C.c_size_t()
        st = lib().gf_file_read_points_elems(ctx.handle, self._h, _ptr(image), image.size, n, _ptr(rows), _ptr(cols), int(bool(verify_checksums)),
                                             max_tiles, _ptrs(out), _ptr(status), C.byref(touched))
        self._points_done("gf_file_read_points_elems", st, return_code)
        return (out, status, touched.value) + ((st,) if return_code else ())

    @staticmethod
    def _interp_names(target):
        return ["z"] + (["zx", "zy"] if target >= INTERP_FIRST else []) + (["zxx", "zxy", "zyy"] if target >= INTERP_SECOND else [])

    def interp_points_dev(self, ctx, elem, spec, rows, cols, col_spacing=None, verify_checksums=True, image=None, max_tiles=None,
                          return_code=False):
        """gf_file_interp_points_dev: B-spline interpolation of element elem at the query points, from the file image in device
        memory (uploaded here); of spec (points_spec()) wrap, target, spacings and fringes are read.  Returns (the dict
        GvrsHipContext.interp_points returns, the touched tiles' count); return_code: ERR_CAPACITY does not raise and (..., the
        call's status) is returned, the outputs as they were pre-set (every byte 0x7f) where the call wrote nothing."""
        image = self.image if image is None else np.frombuffer(bytes(image), np.uint8)
        rows, cols = np.ascontiguousarray(rows, np.float64).ravel(), np.ascontiguousarray(cols, np.float64).ravel()
        assert rows.size == cols.size
        n, target = rows.size, int(spec["target"][0])
        cs = None if col_spacing is None else np.ascontiguousarray(col_spacing, np.float64).ravel()
        assert cs is None or cs.size == n
        max_tiles = self.interp_tiles(spec, rows, cols).size if max_tiles is None else int(max_tiles)
        sizes = {k: n * 8 for k in self._interp_names(target)}
        if target >= INTERP_FIRST:
            sizes["normal"] = n * 24
        sizes["status"] = n * 4
        touched = C.c_size_t()
        with _DeviceScope(ctx) as s:
            d_image = s.upload(image, slack=32, fill=0)
            d_rows, d_cols = s.upload(rows, slack=16), s.upload(cols, slack=16)
            d_cs = None if cs is None else s.upload(cs, slack=16)
            d_out = {k: s.alloc(b + 16, fill=0x7f) for k, b in sizes.items()}
            o = _out_struct(_INTERP_OUT, {k: b.ptr for k, b in d_out.items()})
            st = lib().gf_file_interp_points_dev(ctx.handle, self._h, d_image.ptr, image.size, int(elem), _ptr(spec), n, d_rows.ptr, d_cols.ptr,
                                                 None if d_cs is None else d_cs.ptr, int(bool(verify_checksums)), max_tiles, _ptr(o),
                                                 C.byref(touched))
            self._points_done("gf_file_interp_points_dev", st, return_code)
            ctx.synchronize()
            res = {k: d_out[k].download(np.int32 if k == "status" else np.float64, sizes[k] // (4 if k == "status" else 8)) for k in sizes}
            if "normal" in res:
                res["normal"] = res["normal"].reshape(n, 3)
            return (res, touched.value) + ((st,) if return_code else ())

    def interp_points(self, ctx, elem, spec, rows, cols, col_spacing=None, verify_checksums=True, image=None, max_tiles=None, return_code=False):
        """The same through gf_file_interp_points, the host-memory form."""
        image = self.image if image is None else np.frombuffer(bytes(image), np.uint8)
        rows, cols = np.ascontiguousarray(rows, np.float64).ravel(), np.ascontiguousarray(cols, np.float64).ravel()
        assert rows.size == cols.size
        n, target = rows.size, int(spec["target"][0])
        cs = None if col_spacing is None else np.ascontiguousarray(col_spacing, np.float64).ravel()
        assert cs is None or cs.size == n
        max_tiles = self.interp_tiles(spec, rows, cols).size if max_tiles is None else int(max_tiles)
        res = {k: np.full(n, 0x7f, np.uint8).repeat(8).view(np.float64) for k in self._interp_names(target)}
        if target >= INTERP_FIRST:
            res["normal"] = np.full(n * 3, 0x7f, np.uint8).repeat(8).view(np.float64).reshape(n, 3)
        res["status"] = np.full(n, 0x7f7f7f7f, np.int32)
        o = _out_struct(_INTERP_OUT, {k: a.ctypes.data for k, a in res.items()})
        touched = C.c_size_t()
        st = lib().gf_file_interp_points(ctx.handle, self._h, _ptr(image), image.size, int(elem), _ptr(spec), n, _ptr(rows), _ptr(cols),
                                         None if cs is None else _ptr(cs), int(bool(verify_checksums)), max_tiles, _ptr(o), C.byref(touched))
        self._points_done("gf_file_interp_points", st, return_code)
        return (res, touched.value) + ((st,) if return_code else ())

    # ---- queries at coordinates (gf_file_interp_spec, gf_file_map_points[_dev], gf_file_interp_coords_tiles, gf_file_interp_coords[_dev]) ----
    def coords_spec(self, elem=0, target=INTERP_VALUE):
        """gf_file_interp_spec: the gf_interp_spec the reference's interpolator works with on this file, every field from the file:
        wrap (checkGeographicCoverage), row_spacing = dv, col_spacing = du and the four fringes."""
        s = np.zeros(1, _INTERP_SPEC)
        _call("gf_file_interp_spec", self._h, int(elem), int(target), _ptr(s))
        return s

    @staticmethod
    def _ab(a, b):
        a, b = np.ascontiguousarray(a, np.float64).ravel(), np.ascontiguousarray(b, np.float64).ravel()
        assert a.size == b.size
        return a, b

    def map_points(self, kind, a, b):
        """gf_file_map_points (host arithmetic).  To-grid kinds (MAP_GEO_TO_GRID, MAP_MODEL_TO_GRID): (a, b) = (x, y), x the longitude
        and y the latitude -> dict(row, col, irow, icol, col_spacing, status).  From-grid kinds: (a, b) = (row, col) -> dict(x, y)."""
        a, b = self._ab(a, b)
        n = a.size
        oa, ob = (np.full(n, 0x7f, np.uint8).repeat(8).view(np.float64) for _ in range(2))
        if kind >= MAP_GRID_TO_GEO:
            _call("gf_file_map_points", self._h, int(kind), n, _ptr(a), _ptr(b), _ptr(oa), _ptr(ob), None, None, None, None)
            return {"x": oa, "y": ob}
        ir, ic, st = (np.full(n, 0x7f7f7f7f, np.int32) for _ in range(3))
        cs = np.full(n, 0x7f, np.uint8).repeat(8).view(np.float64)
        _call("gf_file_map_points", self._h, int(kind), n, _ptr(a), _ptr(b), _ptr(oa), _ptr(ob), _ptr(ir), _ptr(ic), _ptr(cs), _ptr(st))
        return {"row": oa, "col": ob, "irow": ir, "icol": ic, "col_spacing": cs, "status": st}

    def map_points_dev(self, ctx, kind, a, b):
        """The same through gf_file_map_points_dev (k_coords_map): the arrays are uploaded here, the call only enqueues."""
        a, b = self._ab(a, b)
        n = a.size
        to_grid = kind < MAP_GRID_TO_GEO
        with _DeviceScope(ctx) as s:
            d_a, d_b = s.upload(a, slack=16), s.upload(b, slack=16)
            d_oa, d_ob = s.alloc(n * 8 + 16, fill=0x7f), s.alloc(n * 8 + 16, fill=0x7f)
            d_ir, d_ic, d_st = ((s.alloc(n * 4 + 16, fill=0x7f) for _ in range(3)) if to_grid else (None, None, None))
            d_cs = s.alloc(n * 8 + 16, fill=0x7f) if to_grid else None
            s.run("gf_file_map_points_dev", ctx.handle, self._h, int(kind), n, d_a.ptr, d_b.ptr, d_oa.ptr, d_ob.ptr,
                  *(x.ptr if x is not None else None for x in (d_ir, d_ic, d_cs, d_st)))
            ctx.synchronize()
            oa, ob = d_oa.download(np.float64, n), d_ob.download(np.float64, n)
            if not to_grid:
                return {"x": oa, "y": ob}
            return {"row": oa, "col": ob, "irow": d_ir.download(np.int32, n), "icol": d_ic.download(np.int32, n),
                    "col_spacing": d_cs.download(np.float64, n), "status": d_st.download(np.int32, n)}

    def interp_coords_tiles(self, kind, spec, a, b):
        """gf_file_interp_coords_tiles: the distinct tiles the windows of the points touch, ascending; the points given as kind says
        (COORDS_GRID: rows, columns; COORDS_FILE: x, y).  A point the latitude check refuses touches none."""
        a, b = self._ab(a, b)
        return self._touched("gf_file_interp_coords_tiles", (self._h, int(kind), _ptr(spec)), a, b)

    def interp_coords_dev(self, ctx, elem, kind, spec, a, b, col_spacing=None, verify_checksums=True, image=None, max_tiles=None,
                          return_code=False):
        """gf_file_interp_coords_dev: interp_points_dev for points given as kind says, mapped inside the kernels; spec is normally
        coords_spec().  col_spacing None: the file's column-spacing rule.  Returns (the dict interp_points_dev returns plus
        col_spacing_used, the touched tiles' count) and with return_code the call's status."""
        image = self.image if image is None else np.frombuffer(bytes(image), np.uint8)
        a, b = self._ab(a, b)
        n, target = a.size, int(spec["target"][0])
        cs = None if col_spacing is None else np.ascontiguousarray(col_spacing, np.float64).ravel()
        assert cs is None or cs.size == n
        max_tiles = self.interp_coords_tiles(kind, spec, a, b).size if max_tiles is None else int(max_tiles)
        sizes = {k: n * 8 for k in self._interp_names(target)}
        if target >= INTERP_FIRST:
            sizes["normal"] = n * 24
        sizes["status"] = n * 4
        touched = C.c_size_t()
        with _DeviceScope(ctx) as s:
            d_image = s.upload(image, slack=32, fill=0)
            d_a, d_b = s.upload(a, slack=16), s.upload(b, slack=16)
            d_cs = None if cs is None else s.upload(cs, slack=16)
            d_out = {k: s.alloc(v + 16, fill=0x7f) for k, v in sizes.items()}
            d_used = s.alloc(n * 8 + 16, fill=0x7f)
            o = _out_struct(_INTERP_OUT, {k: v.ptr for k, v in d_out.items()})
            st = lib().gf_file_interp_coords_dev(ctx.handle, self._h, d_image.ptr, image.size, int(elem), int(kind), _ptr(spec), n, d_a.ptr,
                                                 d_b.ptr, None if d_cs is None else d_cs.ptr, int(bool(verify_checksums)), max_tiles, _ptr(o),
                                                 d_used.ptr, C.byref(touched))
            self._points_done("gf_file_interp_coords_dev", st, return_code)
            ctx.synchronize()
            res = {k: d_out[k].download(np.int32 if k == "status" else np.float64, sizes[k] // (4 if k == "status" else 8)) for k in sizes}
            if "normal" in res:
                res["normal"] = res["normal"].reshape(n, 3)
            res["col_spacing_used"] = d_used.download(np.float64, n)
            return (res, touched.value) + ((st,) if return_code else ())

    def interp_coords(self, ctx, elem, kind, spec, a, b, col_spacing=None, verify_checksums=True, image=None, max_tiles=None, return_code=False):
        """The same through gf_file_interp_coords, the host-memory form."""
        image = self.image if image is None else np.frombuffer(bytes(image), np.uint8)
        a, b = self._ab(a, b)
        n, target = a.size, int(spec["target"][0])
        cs = None if col_spacing is None else np.ascontiguousarray(col_spacing, np.float64).ravel()
        assert cs is None or cs.size == n
        max_tiles = self.interp_coords_tiles(kind, spec, a, b).size if max_tiles is None else int(max_tiles)
        res = {k: np.full(n, 0x7f, np.uint8).repeat(8).view(np.float64) for k in self._interp_names(target)}
        if target >= INTERP_FIRST:
            res["normal"] = np.full(n * 3, 0x7f, np.uint8).repeat(8).view(np.float64).reshape(n, 3)
        res["status"] = np.full(n, 0x7f7f7f7f, np.int32)
        o = _out_struct(_INTERP_OUT, {k: v.ctypes.data for k, v in res.items()})
        res["col_spacing_used"] = np.full(n, 0x7f, np.uint8).repeat(8).view(np.float64)
        touched = C.c_size_t()
        st = lib().gf_file_interp_coords(ctx.handle, self._h, _ptr(image), image.size, int(elem), int(kind), _ptr(spec), n, _ptr(a), _ptr(b),
                                         None if cs is None else _ptr(cs), int(bool(verify_checksums)), max_tiles, _ptr(o),
                                         _ptr(res["col_spacing_used"]), C.byref(touched))
        self._points_done("gf_file_interp_coords", st, return_code)
        return (res, touched.value) + ((st,) if return_code else ())

    def read_coords(self, ctx, x, y, verify_checksums=True, image=None):
        """GvrsElement.readValue(GridPoint) at coordinates (x, y) as z() reads them: map_points (MAP_GEO_TO_GRID for a geographic
        file, MAP_MODEL_TO_GRID otherwise), then read_points at the GridPoint's integer row and column.  Returns ([values [n] per
        element], the cells' status [n_elems, n], the mapping's status [n]); a point the mapping refuses, or whose GridPoint lies
        outside the grid, carries ERR_ARG in the cells' status and the fill."""
        kind = MAP_GEO_TO_GRID if self.info["coordinate_system"] == 2 else MAP_MODEL_TO_GRID
        m = self.map_points(kind, x, y)
        irow = np.where(m["status"] == 0, m["irow"], -1).astype(np.int32)        # (a refused point: outside the grid)
        values, status, _ = self.read_points(ctx, irow, m["icol"], verify_checksums, image)
        return values, status, m["status"]

    # ---- files written (gf_file_assemble, gf_file_write_block_elems[_dev]) ----
    @staticmethod
    def assemble(facts, records, tile_indices, flags=0, image_cap=None, return_code=False):
        """gf_file_assemble: the image of a new file from facts (a GvrsFileFacts) and tile records (list[bytes], b"" for none) of the
        tiles tile_indices, laid in that order -> bytes.  return_code (with image_cap, the room given): (status, image bytes as far
        as the room reaches, the size the image has or needs)."""
        blob, offsets = _blob_of([bytes(r) for r in records])
        idx = np.ascontiguousarray(tile_indices, np.int32)
        assert idx.size == len(records)
        need = C.c_uint64()
        fn = lib().gf_file_assemble
        a = facts.args() + (int(flags), _ptr(blob), _ptr(offsets), _ptr(idx), idx.size)
        if image_cap is None:
            st = fn(*a, None, 0, C.byref(need))
            if st != _lib.ERR_CAPACITY:
                check(st, "gf_file_assemble")
            image_cap = need.value
        image = np.full(max(int(image_cap), 1), 0xA5, np.uint8)
        st = fn(*a, _ptr(image), int(image_cap), C.byref(need))
        if return_code:
            return st, image[:int(image_cap)].tobytes(), need.value
        check(st, "gf_file_assemble")
        return image[:need.value].tobytes()

    @staticmethod
    def _image_dev(ctx, name, head, rect, blocks, mid, cap, n_out, old=None):
        """The device scaffold of write_image and update_image.  Uploads the blocks and a buffer of cap + 64 bytes (old's bytes as
        far as cap reaches, then 0xA5), calls name(ctx, *head, rect, blocks, *mid, image, cap, size, file status, tile indices,
        status, codec used), synchronises, downloads -> (file status, the size the image has or needs, the whole buffer, tile
        indices [n_out], status [n_out], codec used [n_elems, n_out])."""
        ne = len(blocks)
        buf = np.full(cap + 64, 0xA5, np.uint8)
        if old is not None:
            buf[:min(cap, old.size)] = old[:min(cap, old.size)]
        with _DeviceScope(ctx) as s:
            d_blk = [s.upload(b, slack=16) for b in blocks]
            d_image = s.upload(buf)
            d_bytes, d_fst = s.alloc(16, fill=0x7f), s.alloc(16, fill=0x7f)
            d_idx, d_st = s.alloc(n_out * 4 + 16, fill=0x7f), s.alloc(n_out * 4 + 16, fill=0x7f)
            d_used = s.alloc(ne * n_out + 16, fill=0)
            s.run(name, ctx.handle, *head, _ptr(rect), s.ptrs(d_blk), *mid, d_image.ptr, cap, d_bytes.ptr, d_fst.ptr, d_idx.ptr, d_st.ptr, d_used.ptr)
            return (int(d_fst.download(np.int32, 1)[0]), int(d_bytes.download(np.uint64, 1)[0]), d_image.download(np.uint8, cap + 64),
                    d_idx.download(np.int32, n_out), d_st.download(np.int32, n_out), d_used.download(np.uint8, ne * n_out).reshape(ne, n_out))

    @staticmethod
    def _image_host(ctx, name, head, rect, blocks, mid, cap, n_out, old=None):
        """The host scaffold of write_image_host and update_image_host: the image's room of cap bytes (old's bytes, then 0xA5),
        name(ctx, *head, rect, blocks, *mid, image, cap, size, tile indices, status, codec used) -> (the call's return value, the
        size the image has or needs, the room, tile indices, status, codec used)."""
        image = np.full(max(cap, 1), 0xA5, np.uint8)
        if old is not None:
            image[:min(cap, old.size)] = old[:min(cap, old.size)]
        idx, status = np.full(n_out, -1, np.int32), np.full(n_out, 0x7f7f7f7f, np.int32)
        used = np.zeros((len(blocks), n_out), np.uint8)
        need = C.c_uint64()
        rc = getattr(lib(), name)(ctx.handle, *head, _ptr(rect), _ptrs(blocks), *mid, _ptr(image), cap, C.byref(need), _ptr(idx), _ptr(status),
                                  _ptr(used))
        return rc, need.value, image, idx, status, used

    @staticmethod
    def write_image(ctx, facts, blocks, rect=None, flags=0, image_cap=None, raw=False):
        """gf_file_write_block_elems_dev: the image of a new file whose rectangle rect (None: the whole grid) holds blocks (per
        element [n_rows, n_cols]: int32 / int16 / float32, an "icf" element's float VALUES), written in device memory.  Uploads,
        calls, synchronises, downloads: (image bytes, tile indices [n_out], status [n_out], codec used [n_elems, n_out]); raw: (file
        status, the size the image has or needs, the whole buffer of image_cap + 64 bytes pre-filled with 0xA5, tile indices,
        status, codec used) and a file status of ERR_CAPACITY does not raise."""
        rect, n_out = facts.rect_args(rect)
        cap = facts.plan(rect, flags)[1] if image_cap is None else int(image_cap)
        fst, n_bytes, image, idx, status, used = GvrsFileHip._image_dev(ctx, "gf_file_write_block_elems_dev", facts.args(), rect,
                                                                        facts.blocks_in(rect, blocks), (int(flags),), cap, n_out)
        if raw:
            return fst, n_bytes, image, idx, status, used
        check(fst, "gf_file_write_block_elems_dev")
        return image[:n_bytes].tobytes(), idx, status, used

    @staticmethod
    def write_image_host(ctx, facts, blocks, rect=None, flags=0, image_cap=None, return_code=False):
        """The same through gf_file_write_block_elems, the host-memory form, which takes any codec list -> (image bytes, tile indices,
        status, codec used); a negative per-tile status or too small an image_cap raises unless return_code is set: then (the call's
        return value, the size the image has or needs) come first."""
        rect, n_out = facts.rect_args(rect)
        cap = facts.plan(rect, flags)[1] if image_cap is None else int(image_cap)
        rc, need, image, idx, status, used = GvrsFileHip._image_host(ctx, "gf_file_write_block_elems", facts.args(), rect,
                                                                     facts.blocks_in(rect, blocks), (int(flags),), cap, n_out)
        n = min(need, cap)
        if return_code:
            return rc, need, image[:n].tobytes(), idx, status, used
        check(rc, "gf_file_write_block_elems")
        return image[:n].tobytes(), idx, status, used

    # ---- files updated in place (gf_file_update_*) ----
    def update_begin(self, image=None):
        """gf_file_update_begin: the file opened for an update -> a GvrsFileUpdate (the free list after opening, the plan).  image:
        other bytes than the file's own.  A handle serves one image state: after an update, open the new image and begin again."""
        image = self.image if image is None else np.frombuffer(bytes(image), np.uint8)
        return GvrsFileUpdate(self, image)

    def update_assemble(self, upd, records, tile_indices, time_modified, status=None, flags=0, image_cap=None, return_code=False):
        """gf_file_update_assemble: tile records (list[bytes], b"" for none) of the tiles tile_indices applied to the image upd was
        begun on, in that order -> the updated image's bytes.  status: per record, a negative one leaves its tile untouched.
        image_cap: the room given (default: the plan's bound for the whole grid).  return_code: (status, the buffer of image_cap
        bytes -- unchanged behind the old image's bytes, 0xA5, when the call refuses -- and the size the image has or needs)."""
        blob, offsets = _blob_of([bytes(r) for r in records])
        idx = np.ascontiguousarray(tile_indices, np.int32)
        assert idx.size == len(records)
        st = None if status is None else np.ascontiguousarray(status, np.int32)
        cap = upd.plan()[0] if image_cap is None else int(image_cap)
        image = np.full(max(cap, 1), 0xA5, np.uint8)
        image[:min(cap, upd.image.size)] = upd.image[:min(cap, upd.image.size)]
        need = C.c_uint64()
        rc = lib().gf_file_update_assemble(upd.handle, _ptr(image), cap, _ptr(blob), _ptr(offsets), _ptr(idx), None if st is None else _ptr(st),
                                           idx.size, int(time_modified), int(flags), C.byref(need))
        if return_code:
            return rc, image[:cap].tobytes(), need.value
        check(rc, "gf_file_update_assemble")
        return image[:need.value].tobytes()

    def update_records_dev(self, ctx, upd, records, tile_indices, time_modified, status=None, flags=0, image_cap=None, list_capacity=0):
        """gf_file_update_records_dev: update_assemble's device counterpart.  Uploads the image upd was begun on and the records,
        calls, synchronises, downloads -> (file status, the size the image has or needs, the whole buffer of image_cap + 64
        bytes: the old image, then 0xA5).  list_capacity: the room of the allocator's list (0: what the call needs); a list of
        more than 2048 nodes' capacity is worked in the context's scratch, a smaller one in LDS."""
        blob, offsets = _blob_of([bytes(r) for r in records])
        idx = np.ascontiguousarray(tile_indices, np.int32)
        assert idx.size == len(records)
        cap = upd.plan()[0] if image_cap is None else int(image_cap)
        buf = np.full(cap + 64, 0xA5, np.uint8)
        buf[:min(cap, upd.image.size)] = upd.image[:min(cap, upd.image.size)]
        with _DeviceScope(ctx) as s:
            d_image = s.upload(buf)
            d_blob = s.upload(blob, slack=16)
            d_off = s.upload(offsets, slack=16)
            d_idx = s.upload(idx, slack=16)
            d_st = None if status is None else s.upload(np.ascontiguousarray(status, np.int32), slack=16)
            d_bytes = s.alloc(16, fill=0x7f)
            d_fst = s.alloc(16, fill=0x7f)
            s.run("gf_file_update_records_dev", ctx.handle, upd.handle, d_image.ptr, cap, d_blob.ptr, d_off.ptr, d_idx.ptr,
                  None if d_st is None else d_st.ptr, idx.size, int(offsets[-1]), int(time_modified), int(flags), int(list_capacity), d_bytes.ptr,
                  d_fst.ptr)
            return int(d_fst.download(np.int32, 1)[0]), int(d_bytes.download(np.uint64, 1)[0]), d_image.download(np.uint8, cap + 64).tobytes()

    def _update_args(self, upd, rect, blocks, image_cap):
        image0, rect, nt, shape = self._read_args(rect, upd.image)
        blocks = [np.ascontiguousarray(b, dt).reshape(shape) for b, dt in zip(blocks, self._dtypes)]
        assert len(blocks) == self.n_elems
        return image0, rect, nt, blocks, upd.plan(rect)[0] if image_cap is None else int(image_cap)

    def update_image(self, ctx, upd, rect, blocks, time_modified, flags=0, image_cap=None, raw=False):
        """gf_file_update_block_elems_dev: blocks (as update_image_host takes them) stored into rect of the image upd was begun on,
        in device memory.  Uploads, calls, synchronises, downloads: (image bytes, tile indices, status, codec used); raw: (file
        status, the size the image has or needs, the whole buffer of image_cap + 64 bytes -- the old image, then 0xA5 --, tile
        indices, status, codec used), and no file status raises."""
        image0, rect, nt, blocks, cap = self._update_args(upd, rect, blocks, image_cap)
        fst, n_bytes, image, idx, status, used = self._image_dev(ctx, "gf_file_update_block_elems_dev", (upd.handle,), rect, blocks,
                                                                 (int(flags), int(time_modified)), cap, nt, old=image0)
        if raw:
            return fst, n_bytes, image.tobytes(), idx, status, used
        check(fst, "gf_file_update_block_elems_dev")
        return image[:n_bytes].tobytes(), idx, status, used

    def update_image_host(self, ctx, upd, rect, blocks, time_modified, flags=0, image_cap=None, return_code=False):
        """gf_file_update_block_elems: blocks (per element [n_rows, n_cols]: int32 / int16 / float32, an "icf" element's float
        VALUES) stored into rect = (row0, col0, n_rows, n_cols) of the image upd was begun on, in host memory, any codec list ->
        (image bytes, tile indices, status, codec used); a negative per-tile status raises unless return_code is set: then (the
        call's return value, the size the image has or needs) come first."""
        image0, rect, nt, blocks, cap = self._update_args(upd, rect, blocks, image_cap)
        rc, need, image, idx, status, used = self._image_host(ctx, "gf_file_update_block_elems", (upd.handle,), rect, blocks,
                                                              (int(flags), int(time_modified)), cap, nt, old=image0)
        n = min(need, cap) if rc != _lib.ERR_CAPACITY else min(image0.size, cap)
        if return_code:
            return rc, need, image[:n].tobytes(), idx, status, used
        check(rc, "gf_file_update_block_elems")
        return image[:n].tobytes(), idx, status, used

    # ---- writes at scattered points (gf_file_update_plan_tiles, gf_file_update_points_elems[_dev]) ----
    @staticmethod
    def update_plan_tiles(upd, n_tiles):
        """gf_file_update_plan_tiles: GvrsFileUpdate.plan for a count of touched tiles in place of a rectangle -> (the largest
        image an update of that many tiles can need, the free list's capacity for it)."""
        most, cap = C.c_uint64(), C.c_uint64()
        _call("gf_file_update_plan_tiles", upd.handle, int(n_tiles), C.byref(most), C.byref(cap))
        return most.value, cap.value

    def _points_args(self, upd, rows, cols, values, image_cap, max_tiles):
        rows, cols = np.ascontiguousarray(rows, np.int32).ravel(), np.ascontiguousarray(cols, np.int32).ravel()
        assert rows.size == cols.size and len(values) == self.n_elems
        values = [np.ascontiguousarray(v, dt).ravel() for v, dt in zip(values, self._dtypes)]
        assert all(v.size == rows.size for v in values)
        room = self.cells_tiles(rows, cols).size if max_tiles is None else int(max_tiles)
        cap = self.update_plan_tiles(upd, min(room, self.cells_tiles(rows, cols).size))[0] if image_cap is None else int(image_cap)
        return rows, cols, values, room, cap

    def update_points(self, ctx, upd, rows, cols, values, time_modified, flags=0, image_cap=None, max_tiles=None, raw=False):
        """gf_file_update_points_elems_dev: values (per element [n]: int32 / int16 / float32, an "icf" element's float VALUES)
        stored into the cells (rows[i], cols[i]) of the image upd was begun on, in device memory, as element.writeValue point after
        point and close() would.  Uploads, calls, synchronises, downloads: (image bytes, point status [n_elems, n], tile indices
        [t], tile status [t], codec used [n_elems, t]) over the t touched tiles, ascending.  max_tiles: the room in tiles (default:
        the host's count); image_cap: the room of the image (default: the plan's for the touched tiles).  raw: (the call's return
        value, file status, the size the image has or needs, the whole buffer of image_cap + 64 bytes -- the old image, then 0xA5
        --, point status, tile indices [room + 4], tile status [room + 4], codec used [n_elems * room + 16], the touched tiles'
        count), every output pre-set to bytes 0x7f, and nothing raises."""
        rows, cols, values, room, cap = self._points_args(upd, rows, cols, values, image_cap, max_tiles)
        n, ne = rows.size, self.n_elems
        buf = np.full(cap + 64, 0xA5, np.uint8)
        buf[:min(cap, upd.image.size)] = upd.image[:min(cap, upd.image.size)]
        touched = C.c_size_t()
        with _DeviceScope(ctx) as s:
            d_rows, d_cols = s.upload(rows, slack=16), s.upload(cols, slack=16)
            d_val = [s.upload(v, slack=16) for v in values]
            d_image = s.upload(buf)
            d_bytes, d_fst = s.alloc(16, fill=0x7f), s.alloc(16, fill=0x7f)
            d_pst = s.alloc(ne * n * 4 + 16, fill=0x7f)
            d_idx, d_st = s.alloc((room + 4) * 4, fill=0x7f), s.alloc((room + 4) * 4, fill=0x7f)
            d_used = s.alloc(ne * room + 16, fill=0x7f)
            rc = lib().gf_file_update_points_elems_dev(ctx.handle, upd.handle, n, d_rows.ptr, d_cols.ptr, s.ptrs(d_val), room, int(flags),
                                                       int(time_modified), d_image.ptr, cap, d_bytes.ptr, d_fst.ptr, d_pst.ptr, d_idx.ptr,
                                                       d_st.ptr, d_used.ptr, C.byref(touched))
            ctx.synchronize()
            t = touched.value
            fst, n_bytes = int(d_fst.download(np.int32, 1)[0]), int(d_bytes.download(np.uint64, 1)[0])
            image = d_image.download(np.uint8, cap + 64)
            pst = d_pst.download(np.int32, ne * n).reshape(ne, n)
            idx, st, used = d_idx.download(np.int32, room + 4), d_st.download(np.int32, room + 4), d_used.download(np.uint8, ne * room + 16)
        if raw:
            return rc, fst, n_bytes, image.tobytes(), pst, idx, st, used, t
        check(rc, "gf_file_update_points_elems_dev")
        if n:
            check(fst, "gf_file_update_points_elems_dev")
        else:
            n_bytes = upd.image.size                                 # (nothing was enqueued: the image is the old one)
        return image[:n_bytes].tobytes(), pst, idx[:t], st[:t], used[:ne * t].reshape(ne, t)

    def update_points_host(self, ctx, upd, rows, cols, values, time_modified, flags=0, image_cap=None, max_tiles=None, return_code=False):
        """gf_file_update_points_elems: the same through host memory, any codec list -> (image bytes, point status, tile indices,
        tile status, codec used); a negative per-tile status raises unless return_code is set: then (the call's return value, the
        size the image has or needs, the touched tiles' count) come first, and the arrays are whole: tile indices and status
        [room], codec used [n_elems * room], pre-set to bytes 0x7f."""
        rows, cols, values, room, cap = self._points_args(upd, rows, cols, values, image_cap, max_tiles)
        n, ne = rows.size, self.n_elems
        image = np.full(max(cap, 1), 0xA5, np.uint8)
        image[:min(cap, upd.image.size)] = upd.image[:min(cap, upd.image.size)]
        pst = np.full((ne, n), 0x7f7f7f7f, np.int32)
        idx, st = np.full(room + 1, 0x7f7f7f7f, np.int32), np.full(room + 1, 0x7f7f7f7f, np.int32)
        used = np.full(ne * room + 1, 0x7f, np.uint8)
        need, touched = C.c_uint64(), C.c_size_t()
        rc = lib().gf_file_update_points_elems(ctx.handle, upd.handle, n, _ptr(rows), _ptr(cols), _ptrs(values), room, int(flags), int(time_modified),
                                               _ptr(image), cap, C.byref(need), _ptr(pst), _ptr(idx), _ptr(st), _ptr(used), C.byref(touched))
        t = touched.value
        nb = min(need.value, cap) if rc != _lib.ERR_CAPACITY else min(upd.image.size, cap)
        if return_code:
            return rc, need.value, t, image[:nb].tobytes(), pst, idx[:room], st[:room], used[:ne * room]
        check(rc, "gf_file_update_points_elems")
        return image[:nb].tobytes(), pst, idx[:t], st[:t], used[:ne * t].reshape(ne, t)

    # ---- files inspected (gf_file_inspect[_dev]) ----
    def inspect_plan(self, image_bytes=None):
        """gf_file_inspect_plan -> (segment bytes, CRC chunk bytes, the default room for records) of the device form"""
        seg, chunk, most = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _call("gf_file_inspect_plan", self._h, self.image.size if image_bytes is None else int(image_bytes), C.byref(seg), C.byref(chunk), C.byref(most))
        return seg.value, chunk.value, most.value

    def inspect(self, image=None, bad_cap=None, records_cap=None, return_code=False):
        """gf_file_inspect: GvrsInspector's walk over the image in host memory -> a GvrsInspection.  image: other bytes than the
        file's own.  bad_cap / records_cap: the room given (default: what the image needs, found by a first call without
        records); return_code: (status, GvrsInspection) and GF_ERR_CAPACITY does not raise."""
        image = self.image if image is None else np.frombuffer(bytes(image), np.uint8)
        report = np.zeros(1, _FILE_INSPECT_REPORT)
        if bad_cap is None or records_cap is None:
            _call("gf_file_inspect", self._h, _ptr(image), image.size, _ptr(report), None, 0, None, 0)
            bad_cap = int(report[0]["n_bad_tiles"]) if bad_cap is None else bad_cap
            records_cap = int(report[0]["n_records"]) if records_cap is None else records_cap
        bad = np.full(int(bad_cap) + 4, 0x7f7f7f7f, np.int32)
        records = np.full((int(records_cap) + 2) * _FILE_RECORD.itemsize, 0x7f, np.uint8).view(_FILE_RECORD)
        rc = lib().gf_file_inspect(self._h, _ptr(image), image.size, _ptr(report), _ptr(bad), int(bad_cap), _ptr(records), int(records_cap))
        out = GvrsInspection(report[0], bad, int(bad_cap), records, int(records_cap))
        if return_code:
            return rc, out
        check(rc, "gf_file_inspect")
        return out

    def inspect_dev(self, ctx, image=None, max_records=None, bad_cap=None, with_records=True, return_code=False):
        """gf_file_inspect_dev: the same in device memory.  Uploads the image, calls, synchronises, downloads -> a GvrsInspection.
        max_records: the room of the record list (default: the plan's); on GF_ERR_CAPACITY the call is made once more with the
        count the report names, unless return_code: then (the report's status, GvrsInspection) come back as they are.
        bad_cap: the room for bad tiles (default: the grid's tiles)."""
        image = self.image if image is None else np.frombuffer(bytes(image), np.uint8)
        room = self.inspect_plan(image.size)[2] if max_records is None else int(max_records)
        room = max(room, 1)
        n_tiles = -(-self.grid[0] // self.grid[2]) * -(-self.grid[1] // self.grid[3])
        bad_cap = n_tiles if bad_cap is None else int(bad_cap)
        for attempt in range(2):
            with _DeviceScope(ctx) as s:
                d_image = s.upload(image, slack=32, fill=0)
                d_report = s.alloc(_FILE_INSPECT_REPORT.itemsize + 16, fill=0x7f)
                d_bad = s.alloc((bad_cap + 4) * 4, fill=0x7f)
                d_rec = s.alloc((room + 2) * _FILE_RECORD.itemsize, fill=0x7f) if with_records else None
                s.run("gf_file_inspect_dev", ctx.handle, self._h, d_image.ptr, image.size, room, d_report.ptr, d_bad.ptr, bad_cap,
                      None if d_rec is None else d_rec.ptr)
                report = d_report.download(np.uint8, _FILE_INSPECT_REPORT.itemsize + 16)
                bad = d_bad.download(np.int32, bad_cap + 4)
                records = None if d_rec is None else d_rec.download(np.uint8, (room + 2) * _FILE_RECORD.itemsize).view(_FILE_RECORD)
            assert bytes(report[_FILE_INSPECT_REPORT.itemsize:]) == b"\x7f" * 16, "gf_file_inspect_dev wrote behind its report"
            out = GvrsInspection(report[:_FILE_INSPECT_REPORT.itemsize].view(_FILE_INSPECT_REPORT)[0], bad, bad_cap, records, room)
            if return_code or out.status != _lib.ERR_CAPACITY or attempt == 1:
                break
            room = out.n_records
        if return_code:
            return out.status, out
        check(out.status, "gf_file_inspect_dev")
        return out

    def close(self):
        if self._h:
            lib().gf_file_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GvrsInspection:
    """What gf_file_inspect[_dev] answered: the report's fields as attributes (status, failed, complete, stop, stop_name,
    bad_tile_index, invalid_record_size, tile_dir_located, tile_dir_passed, termination_pos, n_records, n_by_type,
    n_checksum_failures, n_bad_tiles), .bad_tiles (the first bad_cap of them, in file order), .records ([(pos, size, type, tile
    index, checksum)], None where none were asked for or the room was too small) and .guards_intact: the entries behind
    bad_cap and records_cap are as they were."""

    def __init__(self, report, bad, bad_cap, records, records_cap):
        for k in _FILE_INSPECT_REPORT.names:
            v = report[k]
            setattr(self, k, [int(x) for x in v] if v.ndim else int(v))
        self.stop_name = INSPECT_STOPS[self.stop] if 0 <= self.stop < len(INSPECT_STOPS) else None
        self.passed = self.status == 0 and not self.failed
        n_bad = min(self.n_bad_tiles, bad_cap)
        self.bad_tiles = [int(t) for t in bad[:n_bad]]
        guard = np.full(1, 0x7f7f7f7f, np.int32)[0]
        self.guards_intact = bool((bad[n_bad:] == guard).all())
        self.records = self.records_raw = None
        if records is not None:
            n = min(self.n_records, records_cap)                  # (the host form fills the room it has)
            raw = records.view(np.uint8).reshape(-1, _FILE_RECORD.itemsize)
            self.records_raw = raw
            self.guards_intact = self.guards_intact and bool((raw[n:] == 0x7f).all())
            if self.status == 0 and self.n_records <= records_cap:
                self.records = [tuple(int(records[k][f]) for f in _FILE_RECORD.names) for k in range(n)]

    def report(self):
        return {k: getattr(self, k) for k in _FILE_INSPECT_REPORT.names}


class GvrsFileUpdate:
    """A file opened for an update (gf_file_update_begin): .free_list = [(position, size)] after the three deallocations of
    opening, plan(rect) = (the largest image an update of the rectangle's tiles can need, the free list's capacity for it)."""

    def __init__(self, file, image):
        self.file, self.image = file, image
        self.handle = C.c_void_p()
        _call("gf_file_update_begin", file._h, _ptr(image), image.size, C.byref(self.handle))
        n = C.c_size_t()
        rc = lib().gf_file_update_free_list(self.handle, None, None, 0, C.byref(n))
        if rc != _lib.ERR_CAPACITY:
            check(rc, "gf_file_update_free_list")
        pos, size = np.zeros(max(n.value, 1), np.uint64), np.zeros(max(n.value, 1), np.uint64)
        _call("gf_file_update_free_list", self.handle, _ptr(pos), _ptr(size), n.value, C.byref(n))
        self.free_list = [(int(p), int(z)) for p, z in zip(pos[:n.value], size[:n.value])]

    def plan(self, rect=None):
        r = None if rect is None else np.ascontiguousarray(rect, np.int32)
        most, cap = C.c_uint64(), C.c_uint64()
        _call("gf_file_update_plan", self.handle, None if r is None else _ptr(r), C.byref(most), C.byref(cap))
        return most.value, cap.value

    def end(self):
        if self.handle:
            lib().gf_file_update_end(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.end()
        except Exception:
            pass
