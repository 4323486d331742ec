"""The library's scratch plan (gf_internal_scratch_plan, gf_internal_scratch_reserve: gvrs_api_route.hip) and a context's scratch
sizes (gf_internal_context_scratch, gvrs_api.hip) through ctypes.  The plan is a pure host function: it needs no device."""
import ctypes as C

from route_plan import KIND_CANON, KIND_HUFFMAN, KIND_RAW_M32

KIND_LSOP_DEC, KIND_LSOP_ENC = 5, 6
BUFFERS = ("workspace", "trees", "packRecs")
# the parts of each buffer (gf_scratch_plan)
PARTS = {"trees": ("leaf", "spare", "roomy", "lengths", "slack", "lsop0", "lsop1"), "packRecs": ("sel", "stats", "plane", "hist")}


class Part(C.Structure):
    _fields_ = [("at", C.c_uint64), ("bytes", C.c_uint64)]


class Plan(C.Structure):
    _fields_ = ([(b, C.c_uint64) for b in BUFFERS] + [("wsStride", C.c_uint64), ("planeStride", C.c_uint64)] +
                [(p, Part) for b in ("trees", "packRecs") for p in PARTS[b]])


_L = None


def lib():
    global _L
    if _L is None:
        from gridfour_amd import _lib
        L = _lib.lib()
        L.gf_internal_scratch_plan.restype = C.c_int
        L.gf_internal_scratch_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.POINTER(Plan)]
        L.gf_internal_scratch_plan_bytes.restype = C.c_size_t
        L.gf_internal_scratch_reserve.restype = C.c_int
        L.gf_internal_scratch_reserve.argtypes = [C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_uint64)]
        L.gf_internal_context_scratch.restype = C.c_int
        L.gf_internal_context_scratch.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        assert L.gf_internal_scratch_plan_bytes() == C.sizeof(Plan)
        _L = L
    return _L


def plan(kind, n_rows, n_cols, n_tiles, lean=0, via_fast=0):
    p = Plan()
    s = lib().gf_internal_scratch_plan(kind, n_rows, n_cols, n_tiles, lean, via_fast, C.byref(p))
    assert s == 0, (kind, n_rows, n_cols, n_tiles, s)
    return p


def reserve(n_rows, n_cols, n_tiles):
    """the bytes gf_context_reserve asks of (workspace, trees, packRecs)"""
    out = (C.c_uint64 * 3)()
    assert lib().gf_internal_scratch_reserve(n_rows, n_cols, n_tiles, out) == 0
    return tuple(out)


def context_scratch(ctx):
    """(bytes held of workspace, trees, packRecs), bytes of all the context's device buffers, moves of its buffers"""
    out = (C.c_uint64 * 5)()
    assert lib().gf_internal_context_scratch(ctx.handle, out) == 0
    return tuple(out[:3]), out[3], out[4]


def variants():
    """(kind, lean, viaFast) of every form the launch sites ask the plan for"""
    for kind in (KIND_HUFFMAN, KIND_RAW_M32, KIND_LSOP_DEC, KIND_LSOP_ENC):
        for lean in (0, 1):
            yield kind, lean, 0
    for lean in (0, 1):
        for via_fast in (0, 1):
            yield KIND_CANON, lean, via_fast
