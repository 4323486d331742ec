"""The library's route plan (gf_internal_route_plan, gvrs_api_route.hip) and route report (gf_internal_route_report) through ctypes,
and the tile-shape sweep the route tests share.  The plan is a pure host function: it needs the library, not a device."""
import ctypes as C

KIND_HUFFMAN, KIND_CANON, KIND_RAW_M32 = 0, 1, 2
# k_huffman_decode<MODE>: bit 3 * MODE + build (gvrs_kernels.h, gf_rt_dec_bit)
DEC_GENERAL, DEC_ANALYZE, DEC_FAST, DEC_FAST_ROOMY, DEC_FAST_CANON = range(5)
MODES = {DEC_GENERAL: "DEC_GENERAL", DEC_ANALYZE: "DEC_ANALYZE", DEC_FAST: "DEC_FAST", DEC_FAST_ROOMY: "DEC_FAST_ROOMY",
         DEC_FAST_CANON: "DEC_FAST_CANON"}
BUILDS = (256, 512, 1024)
CANON_DEC_T256, CANON_DEC_T512, CANON_ANALYZE = 1 << 15, 1 << 16, 1 << 17
TREES_1, TREES_64, LENGTHS_1, LENGTHS_64 = 1 << 18, 1 << 19, 1 << 20, 1 << 21
ENC_SPLIT, ENC_FAST, ENC_GENERAL, ENC_PACK, ENC_PACK_RARE, ENC_LEAN_T1024 = (1 << k for k in range(6))
CANON_ENC_1, CANON_ENC_0, CANON_PACK, ENC_PLANE = 1 << 6, 1 << 7, 1 << 8, 1 << 9
ROOMY_NONE, ROOMY_BESIDE, ROOMY_BEHIND, ROOMY_SKIPPED = range(4)
MAX_CELLS = 1 << 28                      # encodeBatchDev / decodeBatchDev: GF_ERR_UNSUPPORTED from here on
LEAN_MAX_CELLS = ((1 << 23) - 1) // 6    # the one-tile encoder's 1024-thread build: 6 * cells < 2^23


def dec_bit(mode, threads):
    return 1 << (3 * mode + BUILDS.index(threads))


class Plan(C.Structure):
    _fields_ = [("decThreads", C.c_int32), ("viaFast", C.c_int32), ("fastM32", C.c_uint32), ("ldsM32Roomy", C.c_uint32),
                ("canonThreads", C.c_int32), ("prepass", C.c_int32), ("roomyForm", C.c_int32), ("leanEncode", C.c_int32),
                ("decBits", C.c_uint32), ("encBits", C.c_uint32)]


class Report(C.Structure):
    _fields_ = [("encBits", C.c_uint32), ("decBits", C.c_uint32), ("encKind", C.c_int32), ("decKind", C.c_int32),
                ("roomyForm", C.c_int32), ("prepass", C.c_int32), ("roomySeen", C.c_uint32), ("pad", C.c_uint32),
                ("flags", C.c_uint32 * 8)]


_L = None


def lib():
    global _L
    if _L is None:
        from gridfour_amd import _lib
        L = _lib.lib()
        L.gf_internal_route_plan.restype = C.c_int
        L.gf_internal_route_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.POINTER(Plan)]
        L.gf_internal_route_plan_bytes.restype = C.c_size_t
        L.gf_internal_route_report.restype = C.c_int
        L.gf_internal_route_report.argtypes = [C.c_void_p, C.POINTER(Report)]
        L.gf_internal_route_report_bytes.restype = C.c_size_t
        L.gf_internal_decode_lds_per_wg.restype = C.c_size_t
        L.gf_internal_decode_lds_per_wg.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32]
        assert L.gf_internal_route_plan_bytes() == C.sizeof(Plan)
        assert L.gf_internal_route_report_bytes() == C.sizeof(Report)
        _L = L
    return _L


def plan(kind, n_rows, n_cols, n_tiles=1024, lean=0, analysis=0, roomy_seen=0):
    p = Plan()
    s = lib().gf_internal_route_plan(kind, n_rows, n_cols, n_tiles, lean, analysis, roomy_seen, C.byref(p))
    if s != 0:
        raise ValueError("gf_internal_route_plan(%d, %d, %d): status %d" % (kind, n_rows, n_cols, s))
    return p


def report(ctx):
    """what ctx's last encode and decode batches launched; call after ctx.synchronize()"""
    r = Report()
    s = lib().gf_internal_route_report(ctx.handle, C.byref(r))
    assert s == 0, s
    return r


def sweep():
    """squares 1..320, then tall and wide strips up to the 2^28-cell limit (sweep order: what 'first' and 'last' refer to)"""
    shapes = [(n, n) for n in range(1, 321)]
    for j in range(29):
        for k in (2 ** j - 1, 2 ** j, 2 ** j + 1):
            for short in (1, 2, 3, 4, 255, 256, 257):
                for shape in ((k, short), (short, k)):
                    if k >= 1 and shape[0] * shape[1] < MAX_CELLS:
                        shapes.append(shape)
    # the encoder's lean edge, the canonical 512-thread edge and the fast run's LDS edge in a few forms
    for cells in (LEAN_MAX_CELLS, LEAN_MAX_CELLS + 1, 6999, 7000):
        shapes += [(1, cells), (cells, 1)]
    shapes += [(2, LEAN_MAX_CELLS // 2), (2, LEAN_MAX_CELLS // 2 + 1), (70, 100), (3, 2333), (383, 256), (384, 256)]
    seen, out = set(), []
    for s in shapes:
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


VARIANTS = {"huffman": (KIND_HUFFMAN, 0, 0), "lean": (KIND_HUFFMAN, 1, 0), "analyze": (KIND_HUFFMAN, 0, 1), "deflate": (KIND_RAW_M32, 0, 0),
            "canon": (KIND_CANON, 0, 0), "canon-lean": (KIND_CANON, 1, 0), "canon-analyze": (KIND_CANON, 0, 1)}


def domains(shapes=None):
    """{"<variant>:<instantiation>": [shapes of the sweep that launch it, in sweep order]} for the decode and encode matrix;
    variant: a CodecHuffman batch, the one-tile path (lean), analysis, CodecDeflate (raw M32) and the canonical forms"""
    shapes = sweep() if shapes is None else shapes
    dom = {}

    def add(name, shape):
        dom.setdefault(name, []).append(shape)

    for r, c in shapes:
        for var, (kind, lean, analysis) in VARIANTS.items():
            p = plan(kind, r, c, 1024, lean, analysis)
            for mode in MODES:
                for b in BUILDS:
                    if p.decBits & dec_bit(mode, b):
                        add("%s:%s/%d" % (var, MODES[mode], b), (r, c))
            for bit, name in ((CANON_DEC_T256, "k_canon_decode/256"), (CANON_DEC_T512, "k_canon_decode/512"),
                              (CANON_ANALYZE, "k_canon_decode<true>"), (TREES_1, "k_huffman_parse_trees<1>"),
                              (LENGTHS_1, "k_canon_parse_lengths<1>")):
                if p.decBits & bit:
                    add("%s:%s" % (var, name), (r, c))
            for bit, name in ((ENC_SPLIT, "k_huffman_encode<true,1>"), (ENC_FAST, "k_huffman_encode<true>"),
                              (ENC_GENERAL, "k_huffman_encode<false>"), (ENC_PACK_RARE, "k_huffman_pack_rare"),
                              (ENC_LEAN_T1024, "encode_t1024"), (CANON_ENC_1, "k_canon_encode<1>"), (CANON_ENC_0, "k_canon_encode<0>")):
                if p.encBits & bit:
                    add("%s:%s" % (var, name), (r, c))
    return dom


def reached(dom, name):
    """the variants' domains of one instantiation, merged"""
    return [s for k, v in dom.items() if k.split(":", 1)[1] == name for s in v]


def square_ends(dom, name, min_cells=1, max_cells=1 << 16):
    """first and last square of an instantiation's domain within the sweep, among squares of 2x2 and min_cells..max_cells cells
    ([None] where there is none: the caller's test fails on it)"""
    sq = [s for s in dom.get(name, []) if s[0] == s[1] >= 2 and min_cells <= s[0] * s[1] <= max_cells]
    if not sq:
        return [None]
    return [sq[0], sq[-1]] if sq[-1] != sq[0] else [sq[0]]


def roomy_tiles(r, c, n, seed, p):
    """tiles whose M32 stream outgrows the fast run's buffer and fits the roomy one (plan p): small noise with spikes of 450 (two
    M32 bytes) at a density chosen on the oracle's packing of the first tile"""
    import numpy as np
    import oracle
    for q in (0.2, 0.12, 0.06):
        rng = np.random.default_rng(seed + r * 7 + c)
        tiles = [(rng.integers(0, 4, r * c) + 450 * (rng.random(r * c) < q)).astype(np.int32) for _ in range(n)]
        n_m32 = int.from_bytes(oracle.codec_huffman_encode(0, r, c, tiles[0])[0][6:10], "little")
        if p.fastM32 < n_m32 <= p.ldsM32Roomy - 4096:
            return tiles
    raise AssertionError("no spike density puts a %dx%d tile between the fast and the roomy budget" % (r, c))


DEM_SEED = 0x5EED_0F_2047                  # the synthetic terrain of device_roundtrip(style=...)


def sampled(n, k=23):
    """about k tile indices spread over n"""
    return range(0, n, max(1, n // k))


def _oracle_encode(kind, r, c, tile, predictor_mask=0xF):
    import oracle
    f = oracle.codec_canon_encode if kind == KIND_CANON else oracle.codec_huffman_encode
    return f(0, r, c, tile, predictor_mask=predictor_mask)


def device_roundtrip(ctx, kind, r, c, tiles=None, style=None, n_tiles=None, sample=None, check_decode=True, slot_stride=None,
                    seed=DEM_SEED, predictor_mask=0xF):
    """values -> encode -> decode on one DeviceTileBatch (one encodeBatchDev and one decodeBatchDev call), against the oracle;
    returns (batch, report after encode, report after decode, plan of the decode)"""
    import gridfour_amd
    import numpy as np
    nt = len(tiles) if tiles is not None else n_tiles
    b = gridfour_amd.DeviceTileBatch(ctx, r, c, nt, slot_stride=slot_stride, codec="canon" if kind == KIND_CANON else "huffman")
    if tiles is not None:
        b.values.upload(np.ascontiguousarray(np.stack(tiles), dtype=np.int32))
    else:
        b.synth_dem(seed, 144, style=style)
    b.encode(codec_index=0, predictor_mask=predictor_mask)
    ctx.synchronize()
    enc = report(ctx)
    vals = b.get_values()
    assert (b.get_enc_status() == 0).all()
    lengths, preds = b.get_lengths(), b.get_predictors()
    for t in (range(nt) if sample is None else sampled(nt, sample)):
        ref, used = _oracle_encode(kind, r, c, vals[t], predictor_mask)
        assert preds[t] == used and b.get_packing(t, int(lengths[t])) == ref, ("packing", r, c, t)
    seen = enc.roomySeen                             # the hint the decode's plan reads
    b.decoded.fill(0)
    b.decode()
    ctx.synchronize()
    dec = report(ctx)
    p = plan(kind, r, c, nt, 0, 0, seen)
    if check_decode:
        assert (b.get_dec_status() == 0).all()
        assert np.array_equal(b.get_decoded(), vals), ("decoded", r, c)
    assert enc.encKind == kind and dec.decKind == kind
    assert enc.encBits == p.encBits, (hex(enc.encBits), hex(p.encBits))
    assert dec.decBits == p.decBits, (hex(dec.decBits), hex(p.decBits))
    assert dec.roomyForm == p.roomyForm and dec.prepass == p.prepass
    return b, enc, dec, p
