"""Residuals at the edges of their encoding classes (tests/value_edges.py) through every integer codec path of the library, against
the oracle: packings byte for byte, decoded tiles value for value.  The CodecHuffman, CodecCanonHuffman and raw M32 / Deflate
cases also assert through route_plan.report that the planned kernels ran (a threshold change cannot quietly turn a case into a
test of another path); the LSOP12 kernels are not in the route report, so those cases check values only.

M32 edges: both ends of every CodecM32 length with both signs, -127 / -128, INT_MAX, INT_MIN + 1 and INT_MIN as a genuine residual,
at the stream positions each predictor treats differently and at every byte phase of a dword, a six-byte value first and last.
Canonical edges: both ends of every kind and one past each, target symbols 0 and 255, both ends of the gap between
CanonicalHuffman.java:258 and :395 (the reference reads a gap value back only where -1 has a code; the library must agree)."""
import struct
import zlib

import numpy as np
import pytest

import oracle
import route_plan as rp
import value_edges as ve
from route_plan import KIND_CANON, KIND_HUFFMAN, KIND_RAW_M32
from tilegen import make_tile
from value_edges import DIFF, LINEAR, NULLS, TRIANGLE

pytestmark = pytest.mark.gpu
MODELS = (DIFF, LINEAR, TRIANGLE)
_DOM = {}


def _ctx():
    import gridfour_amd
    return gridfour_amd.GvrsHipContext(0)


def _square(variant, mode, build, min_cells, max_cells=1 << 16):
    """the first square of the sweep the plan gives this k_huffman_decode build (tests/route_plan.py)"""
    if not _DOM:
        _DOM.update(rp.domains([(n, n) for n in range(2, 321)]))
    name = "%s:%s/%d" % (variant, rp.MODES[mode], build)
    sq = rp.square_ends(_DOM, name, min_cells, max_cells)
    assert sq[0] is not None, "the route plan no longer gives %s a square" % name
    return sq[0]


def _max_stride(r, c):
    from gridfour_amd import _lib
    return int(_lib.lib().gf_huffman_max_packing(r, c))


def _retry_word(p):
    return 1 if p.ldsM32Roomy else 0


def _edge_batch(model, r, c, edges):
    """every edge value at every placement (one tile per value), the byte-phase tiles and, for M32 edges, INT_MIN residuals"""
    tiles = [v for v, _ in ve.value_tiles(model, r, c, edges)]
    tiles += [v for v, _, _ in ve.phase_tiles(model, r, c)]
    tiles += [v for m, v, _ in ve.int_min_tiles(r, c) if m == model]
    return tiles


# ---------------------------------------------------------------- CodecHuffman


@pytest.mark.parametrize("build", rp.BUILDS)
def test_huffman_fast_decode_of_edge_values_each_build(build):
    """DEC_FAST: one distinct edge value per tile, otherwise one-byte residuals; encode by the split kernel and the pack kernels
    (the plane included), decode by the fast kernel of the planned build without the general kernel"""
    r, c = _square("huffman", rp.DEC_FAST, build, 1024)
    ctx = _ctx()
    for model in MODELS:
        tiles = _edge_batch(model, r, c, ve.M32_EDGES)
        _, enc, dec, p = rp.device_roundtrip(ctx, KIND_HUFFMAN, r, c, tiles, predictor_mask=1 << (model - 1),
                                             slot_stride=_max_stride(r, c))
        assert p.decThreads == build and dec.decBits & rp.dec_bit(rp.DEC_FAST, build)
        assert enc.encBits & rp.ENC_SPLIT and enc.encBits & rp.ENC_PLANE and enc.encBits & rp.ENC_PACK
        assert dec.flags[_retry_word(p)] == 0, "the general kernel received an edge tile"


@pytest.mark.parametrize("build", rp.BUILDS)
def test_huffman_general_decode_after_retry_each_build(build):
    """DEC_GENERAL: five- and six-byte edge values at most positions outgrow every LDS budget"""
    r, c = _square("huffman", rp.DEC_GENERAL, build, 2048)
    ctx = _ctx()
    for model in MODELS:
        tiles = [ve.general_edge_tile(model, r, c, seed=5000 + s)[0] for s in range(2)] + [ve.value_tiles(model, r, c, [-ve.IMAX])[0][0]]
        _, _, dec, p = rp.device_roundtrip(ctx, KIND_HUFFMAN, r, c, tiles, predictor_mask=1 << (model - 1),
                                           slot_stride=_max_stride(r, c))
        assert p.decThreads == build
        assert dec.flags[_retry_word(p)] != 0, "the wide tiles did not reach the general kernel"



@pytest.mark.parametrize("build", rp.BUILDS)
def test_huffman_roomy_run_behind_each_build(build):
    """DEC_FAST_ROOMY behind the first run: two- and three-byte edge values at a density between the two budgets"""
    r, c = _square("huffman", rp.DEC_FAST_ROOMY, build, 6000)
    ctx = _ctx()
    n = 4
    tiles = [v for v, _ in ve.roomy_edge_tiles(TRIANGLE, r, c, n, rp.plan(KIND_HUFFMAN, r, c, n + 1))]
    tiles.append(ve.value_tiles(TRIANGLE, r, c, [ve.IMAX])[0][0])
    b, _, dec, p = rp.device_roundtrip(ctx, KIND_HUFFMAN, r, c, tiles, predictor_mask=1 << (TRIANGLE - 1))
    assert p.decThreads == build and p.roomyForm == rp.ROOMY_BEHIND
    for t in range(n):
        n_m32 = int.from_bytes(b.get_packing(t, 10)[6:10], "little")
        assert p.fastM32 < n_m32 <= p.ldsM32Roomy, (t, n_m32, p.fastM32, p.ldsM32Roomy)
    assert dec.decBits & rp.dec_bit(rp.DEC_FAST_ROOMY, build) and dec.roomySeen - 1 == n and dec.flags[1] == 0


def test_huffman_roomy_run_beside():
    """the roomy run beside the first one: 4,096 tiles on a fresh context, eight distinct roomy edge tiles over and over"""
    r, c = 120, 150
    ctx = _ctx()
    distinct = [v for v, _ in ve.roomy_edge_tiles(DIFF, r, c, 8, rp.plan(KIND_HUFFMAN, r, c, 4096))]
    tiles = [distinct[t % 8] for t in range(4096)]
    _, _, dec, p = rp.device_roundtrip(ctx, KIND_HUFFMAN, r, c, tiles, predictor_mask=1, sample=8)
    assert dec.roomyForm == rp.ROOMY_BESIDE and dec.decBits & rp.dec_bit(rp.DEC_FAST_ROOMY, p.decThreads)
    assert dec.roomySeen - 1 == 4096 and dec.flags[1] == 0


def test_huffman_pack_rare_with_rare_edge_values():
    """k_huffman_pack_rare: geometric residuals and a few six- and five-byte edge values (their bytes get long codes)"""
    r, c = 120, 150
    ctx = _ctx()
    tiles = [ve.rare_edge_tile(r, c, seed=6000 + k)[0] for k in range(3)] + [make_tile("smooth", r, c, seed=2)]
    _, enc, _, _ = rp.device_roundtrip(ctx, KIND_HUFFMAN, r, c, tiles, predictor_mask=1, slot_stride=_max_stride(r, c))
    assert enc.encBits & rp.ENC_PACK_RARE and 3 <= enc.flags[5] < len(tiles), list(enc.flags)


def test_huffman_general_encoder_past_the_lean_limit():
    """k_huffman_encode<false> on a tile of 2^23 / 6 cells and more with edge values at every placement"""
    r, c = 2, rp.LEAN_MAX_CELLS // 2 + 1
    ctx = _ctx()
    tile = ve.value_tiles(DIFF, r, c, [ve.IMAX])[0][0]
    _, enc, _, _ = rp.device_roundtrip(ctx, KIND_HUFFMAN, r, c, [tile], predictor_mask=1, slot_stride=_max_stride(r, c))
    assert enc.encBits & rp.ENC_GENERAL and not enc.encBits & rp.ENC_SPLIT


def _lean_pack_keeps(res):
    """k_huffman_pack's flat form in the one-tile build (gvrs_encode.hip: STEP_CELLS x maxN x maxLen <= (WIN_WORDS - 2) x 32 with
    1,024 threads x CPT 8 cells and a 4,096-word window): M32 bytes per value x the longest code at most 15 bits; a tile past that
    is left to the batch path (the one-tile launch has no k_huffman_pack_rare behind it)"""
    max_len = int(oracle.huffman_encode(np.frombuffer(oracle.m32_encode_seq(res), np.uint8))[2].max())
    return max(ve.m32_len(x) for x in res) * max_len <= 15


def test_huffman_one_tile_path():
    """the one-tile path on tiles with one wide edge value each (every wide M32 edge): the streams fit the lean build's fast budget,
    so DEC_FAST of the 1024-thread build alone decodes every one; the 1024-thread lean encoder keeps the tiles whose codes fit its
    pack window (all two- and three-byte edges, at a density that keeps their codes short) and the batch path encodes the others"""
    import gridfour_amd
    r, c = 120, 150
    lean = rp.plan(KIND_HUFFMAN, r, c, 1, lean=1)
    batch = rp.plan(KIND_HUFFMAN, r, c, 1)
    ctx = _ctx()
    codec = gridfour_amd.CodecHuffmanHip(context=ctx)
    cases = []
    for k, e in enumerate(sorted(ve.WIDE, key=ve.m32_len)):
        for frac in (0.06, 0.08, 0.1, 0.04, 0.02):
            v, res = ve.dense_tile(DIFF, r, c, [e], frac, seed=8000 + k)
            if _lean_pack_keeps(res) or frac == 0.02:
                break
        cases.append((e, v, res))
    kept = {e for e, _, res in cases if _lean_pack_keeps(res)}
    assert kept == {e for e in ve.WIDE if ve.m32_len(e) <= 3}, sorted(kept)
    for e, v, res in cases:
        ref, used = oracle.codec_huffman_encode(0, r, c, v)
        n_m32 = int.from_bytes(ref[6:10], "little")
        assert used == DIFF and (res == e).sum() >= 300 and n_m32 + 8 <= lean.fastM32, (e, used, n_m32, lean.fastM32)
        assert codec.encode(0, r, c, v) == ref
        assert codec.encode(0, r, c, v) == ref
        ctx.synchronize()
        rep = rp.report(ctx)
        want = lean.encBits if e in kept else batch.encBits
        assert rep.encBits == want, (e, hex(rep.encBits), hex(want))
        for _ in range(3):
            assert np.array_equal(codec.decode(r, c, ref), v)
        ctx.synchronize()
        rep = rp.report(ctx)
        assert rep.decBits == lean.decBits == rp.TREES_1 | rp.dec_bit(rp.DEC_FAST, 1024), (e, hex(rep.decBits))


def test_huffman_nulls_tiles():
    """DifferencingWithNulls: edge values right after run starts and right before nulls"""
    r, c = 60, 90
    ctx = _ctx()
    tiles = [ve.nulls_tile(r, c, ve.M32_EDGES[k::3], seed=1000 + k, bg_seed=k)[0] for k in range(3)]
    b, _, _, _ = rp.device_roundtrip(ctx, KIND_HUFFMAN, r, c, tiles, slot_stride=_max_stride(r, c))
    assert (b.get_predictors() == NULLS).all()


def test_huffman_analyze_sums():
    """gf_huffman_analyze_batch over edge packings against the restatement of CodecHuffman.analyze (test_gpu_analyze)"""
    import gridfour_amd
    from test_gpu_analyze import _expected
    r, c = 60, 90
    codec = gridfour_amd.CodecHuffmanHip()
    packs = []
    for model in MODELS:
        packs += [oracle.codec_huffman_encode(0, r, c, v, predictor_mask=1 << (model - 1))[0] for v in _edge_batch(model, r, c, ve.M32_EDGES)]
    packs += [oracle.codec_huffman_encode(0, r, c, ve.general_edge_tile(LINEAR, r, c)[0], predictor_mask=2)[0]]
    codec.clearAnalysisData()
    status = codec.analyze_batch(r, c, packs)
    assert (np.asarray(status) == 0).all()
    codec.ctx.synchronize()
    rep = rp.report(codec.ctx)
    p = rp.plan(KIND_HUFFMAN, r, c, len(packs), 0, 1)
    assert rep.decKind == KIND_HUFFMAN and rep.decBits == p.decBits and rep.decBits & rp.dec_bit(rp.DEC_ANALYZE, p.decThreads)
    want, want_e = _expected(r, c, packs)
    got = codec.analysis_data()
    for k in range(6):
        have = [int(got[k][f]) for f in ("n_tiles", "n_bytes", "n_symbols", "n_bits_overhead", "n_m32_counted", "sum_length_m32",
                                         "sum_observed_m32")]
        assert have == list(want[k]), (k, have, list(want[k]))
        assert got[k]["sum_entropy_m32"] == pytest.approx(want_e[k], rel=1e-12, abs=1e-12)


# ---------------------------------------------------------------- CodecCanonHuffman


def _canon_shapes():
    """a shape of each k_canon_decode build and one the fast legacy kernel takes first (DEC_FAST_CANON)"""
    a, b = (60, 90), (100, 110)
    assert rp.plan(KIND_CANON, *a).canonThreads == 256 and rp.plan(KIND_CANON, *b).canonThreads == 512
    return [a, b]


@pytest.mark.parametrize("shape", _canon_shapes(), ids=lambda s: "%dx%d" % s)
def test_canon_edges_each_build(shape):
    """k_canon_encode + k_canon_pack, then the fast legacy kernel takes the tiles without escapes (kind-0 edges, target symbols 0
    and 255) and k_canon_decode of the planned build the rest"""
    r, c = shape
    ctx = _ctx()
    for model in MODELS:
        tiles = [v for e, (v, _) in zip(ve.CANON_EDGES, ve.value_tiles(model, r, c, ve.CANON_EDGES)) if not ve.in_gap(e)]
        tiles += [v for v, _, minus_one in ve.gap_tiles(model, r, c) if minus_one]
        _, enc, dec, p = rp.device_roundtrip(ctx, KIND_CANON, r, c, tiles, predictor_mask=1 << (model - 1),
                                             slot_stride=_max_stride(r, c))
        assert enc.encBits & rp.CANON_ENC_1 and enc.encBits & rp.CANON_PACK
        assert dec.decBits & (rp.CANON_DEC_T512 if p.canonThreads == 512 else rp.CANON_DEC_T256)
        assert p.viaFast and dec.decBits & rp.dec_bit(rp.DEC_FAST_CANON, p.decThreads)
        assert dec.flags[0] != 0, "no tile was left to k_canon_decode"


def test_canon_gap_values_unreadable_as_in_the_reference():
    """a gap value over a background without -1: the library writes the oracle's bytes and refuses them with the oracle's status"""
    import gridfour_amd
    r, c = 60, 90
    ctx = _ctx()
    codec = gridfour_amd.CodecCanonHuffmanHip(context=ctx)
    for model in MODELS:
        gap = ve.gap_tiles(model, r, c)
        tiles = [v for v, _, _ in gap]
        _, _, _, _ = rp.device_roundtrip(ctx, KIND_CANON, r, c, tiles, predictor_mask=1 << (model - 1), check_decode=False,
                                         slot_stride=_max_stride(r, c))
        refs = [oracle.codec_canon_encode(0, r, c, v, predictor_mask=1 << (model - 1))[0] for v in tiles]
        vals, st = codec.decode_batch(r, c, refs)
        for k, (v, _, minus_one) in enumerate(gap):
            if minus_one:
                assert st[k] == 0 and np.array_equal(vals[k], v), (model, k)
                continue
            with pytest.raises(IOError) as ex:
                oracle.codec_canon_decode(r, c, refs[k])
            assert st[k] == (-2 if "rc=-2" in str(ex.value) else -1), (model, k, st[k], str(ex.value))


def test_canon_analyze_escape_counts():
    """CodecCanonHuffman.analyze over edge packings: the stats and the escape table against tests/canon_analyze_twin.py"""
    import gridfour_amd
    from canon_analyze_twin import Twin, assert_matches
    r, c = 60, 90
    codec = gridfour_amd.CodecCanonHuffmanHip()
    packs = []
    for model in MODELS:
        packs += [oracle.codec_canon_encode(0, r, c, v, predictor_mask=1 << (model - 1))[0]
                  for v, _ in ve.value_tiles(model, r, c, ve.CANON_EDGES)]
    twin = Twin()
    ok = [twin.analyze(r, c, p) for p in packs]
    codec.clearAnalysisData()
    st = codec.analyze_batch(r, c, packs)
    codec.ctx.synchronize()
    rep = rp.report(codec.ctx)
    p = rp.plan(KIND_CANON, r, c, len(packs), 0, 1)
    assert rep.decKind == KIND_CANON and rep.decBits == p.decBits and rep.decBits & rp.CANON_ANALYZE, (hex(rep.decBits), hex(p.decBits))
    for k, good in enumerate(ok):
        assert (st[k] == 0) == good, (k, st[k])
    assert_matches(codec.analysis_data(), codec.escape_counts(), twin)
    assert all(x > 0 for x in twin.escapes), twin.escapes


# ---------------------------------------------------------------- CodecDeflate


def _dev_decode(ctx, fn, r, c, packs):
    from gridfour_amd import DeviceBuffer, lib
    from gridfour_amd._lib import check
    from test_gpu_inflate import _upload_packings
    nt = len(packs)
    d_blob, d_off, d_len, total = _upload_packings(ctx, packs)
    d_vals, d_st = DeviceBuffer(ctx, nt * r * c * 4), DeviceBuffer(ctx, nt * 4 + 16)
    check(getattr(lib(), fn)(ctx.handle, None, r, c, nt, d_blob.ptr, total + 32, d_off.ptr, 0, d_len.ptr, d_vals.ptr, d_st.ptr), fn)
    ctx.synchronize()
    return d_vals.download(np.int32, nt * r * c).reshape(nt, r * c), d_st.download(np.int32, nt)


def test_deflate_m32_streams_and_decodes():
    """k_m32_streams (gf_m32_encode_batch_i32_dev): the three candidate streams against predictor_encode_int + m32_encode_seq;
    gf_deflate_decode_batch_i32_dev on the oracle's packings; gf_m32_decode_batch_i32_dev on raw containers (header + M32 bytes)"""
    import gridfour_amd
    from gridfour_amd import DeviceBuffer, lib
    r, c = 24, 40
    ctx = _ctx()
    tiles = []
    for model in MODELS:
        tiles += _edge_batch(model, r, c, ve.M32_EDGES)
    n_plain = len(tiles)
    tiles += [ve.nulls_tile(r, c, ve.M32_EDGES[k::2], seed=1000 + k, bg_seed=k)[0] for k in range(2)]
    tiles = np.stack(tiles)
    nt = len(tiles)
    sub = int(lib().gf_m32_max_stream(r, c))
    dv, ds = DeviceBuffer(ctx, tiles.nbytes), DeviceBuffer(ctx, nt * 3 * sub + 16)
    dl, dm, dsd, dst = DeviceBuffer(ctx, nt * 12), DeviceBuffer(ctx, nt * 3), DeviceBuffer(ctx, nt * 4), DeviceBuffer(ctx, nt * 4)
    dv.upload(tiles)
    gridfour_amd._lib.check(lib().gf_m32_encode_batch_i32_dev(ctx.handle, None, r, c, nt, dv.ptr, ds.ptr, sub, dl.ptr, dm.ptr,
                                                               dsd.ptr, dst.ptr), "m32 encode")
    ctx.synchronize()
    lens, models, seeds = dl.download(np.uint32, nt * 3), dm.download(np.uint8, nt * 3), dsd.download(np.int32, nt)
    streams = ds.download(np.uint8, nt * 3 * sub)
    assert (dst.download(np.int32, nt) == 0).all()
    raw = []
    for t in range(n_plain, nt):                # a tile with nulls: the DifferencingWithNulls stream in sub-slot 0
        res, seed = oracle.predictor_encode_int(NULLS, r, c, tiles[t])
        m32 = oracle.m32_encode_seq(res)
        off = t * 3 * sub
        assert models[t * 3] == NULLS and lens[t * 3] == len(m32) and seeds[t] == seed, t
        assert bytes(streams[off:off + len(m32)]) == m32, t
        raw.append((bytes([0, NULLS]) + struct.pack("<iI", seed, len(m32)) + m32, tiles[t]))
    for t in range(n_plain):
        for p in range(3):
            res, seed = oracle.predictor_encode_int(p + 1, r, c, tiles[t])
            m32 = oracle.m32_encode_seq(res)
            off = (t * 3 + p) * sub
            assert models[t * 3 + p] == p + 1 and lens[t * 3 + p] == len(m32) and seeds[t] == seed, (t, p)
            assert bytes(streams[off:off + len(m32)]) == m32, (t, p)
            if p == t % 3:
                raw.append((bytes([0, p + 1]) + struct.pack("<iI", seed, len(m32)) + m32, tiles[t]))
    packs = [oracle.codec_deflate_encode(0, r, c, v)[0] for v in tiles]
    assert [pk[1] for pk in packs[n_plain:]] == [NULLS] * (nt - n_plain)
    vals, st = _dev_decode(ctx, "gf_deflate_decode_batch_i32_dev", r, c, packs)
    assert (st == 0).all() and np.array_equal(vals, tiles)
    rep = rp.report(ctx)                         # (the inflated chunks go through the raw M32 decode)
    assert rep.decKind == KIND_RAW_M32 and rep.decBits == rp.plan(KIND_RAW_M32, r, c, nt).decBits
    vals, st = _dev_decode(ctx, "gf_m32_decode_batch_i32_dev", r, c, [pk for pk, _ in raw])
    ctx.synchronize()
    assert (st == 0).all() and np.array_equal(vals, np.stack([v for _, v in raw]))
    rep = rp.report(ctx)
    assert rep.decKind == KIND_RAW_M32 and rep.decBits == rp.plan(KIND_RAW_M32, r, c, len(raw)).decBits
    # the same M32 text of each predictor's edge stream, raw: the oracle's CodecDeflate decode of the deflated form agrees
    for pk, v in raw[:6]:
        m = pk[10:]
        assert np.array_equal(oracle.codec_deflate_decode(r, c, pk[:10] + zlib.compress(m, 6)), v)
    for b in (dv, ds, dl, dm, dsd, dst):
        b.free()


def test_nulls_sums_on_the_null_code():
    """Hand-made DifferencingWithNulls streams (value_edges.nulls_sum_stream): edge values next to sums that come out as
    Integer.MIN_VALUE without a null residual, in CodecDeflate (host API and gf_deflate_decode_batch_i32_dev), CodecHuffman and
    raw containers (gf_m32_decode_batch_i32_dev), against the oracle's CodecDeflate decode"""
    import gridfour_amd
    r, c = 16, 24
    cases = [ve.nulls_sum_stream(r, c, ve.M32_EDGES[k:] + ve.M32_EDGES[:k], seed=5 + 1000 * k, rng_seed=k) for k in range(6)]
    packs = [ve.nulls_sum_packings(r, c, sd, res) for sd, res, _ in cases]
    want = np.stack([oracle.codec_deflate_decode(r, c, d) for d, _, _ in packs])
    for k, (sd, res, sums) in enumerate(cases):
        assert np.array_equal(oracle.codec_huffman_decode(r, c, packs[k][1]), want[k])
        assert all(want[k][i] == ve.NULL and res[i] != ve.NULL for i in sums) and len(sums) >= r, k
    ctx = _ctx()
    vals, st = gridfour_amd.CodecDeflateHip(context=ctx).decode_batch(r, c, [d for d, _, _ in packs])
    assert (st == 0).all() and np.array_equal(vals, want)
    vals, st = _dev_decode(ctx, "gf_deflate_decode_batch_i32_dev", r, c, [d for d, _, _ in packs])
    assert (st == 0).all() and np.array_equal(vals, want)
    vals, st = _dev_decode(ctx, "gf_m32_decode_batch_i32_dev", r, c, [w for _, _, w in packs])
    assert (st == 0).all() and np.array_equal(vals, want)
    rep = rp.report(ctx)
    assert rep.decKind == KIND_RAW_M32 and rep.decBits == rp.plan(KIND_RAW_M32, r, c, len(packs)).decBits
    ctx = _ctx()
    vals, st = gridfour_amd.CodecHuffmanHip(context=ctx).decode_batch(r, c, [h for _, h, _ in packs])
    ctx.synchronize()
    assert (st == 0).all() and np.array_equal(vals, want)
    rep = rp.report(ctx)
    p = rp.plan(KIND_HUFFMAN, r, c, len(packs))
    assert rep.decKind == KIND_HUFFMAN and rep.decBits == p.decBits, (hex(rep.decBits), hex(p.decBits))


# ---------------------------------------------------------------- LSOP12


def _lsop_packs(nr, nc):
    from test_gpu_lsop import _handmade_type0
    rng = np.random.default_rng(12)
    coefs = (rng.standard_normal(12) * 0.05).astype(np.float32)
    m32 = [e for e in ve.M32_EDGES]
    canon = [e for e in ve.CANON_EDGES if not ve.in_gap(e)]
    packs = []
    for k in range(4):
        init, inter = ve.lsop_streams(nr, nc, m32, k)
        packs.append(_handmade_type0(nr, nc, 100 + k, coefs, init, inter, revised=bool(k & 1), checksum=bool(k & 2)))
        packs.append(ve.lsop_deflate_container(200 + k, coefs, init, inter, checksum=bool(k & 1)))
        init, inter = ve.lsop_streams(nr, nc, canon, k)
        packs.append(ve.lsop_canon_container(300 + k, coefs, init, inter, checksum=bool(k & 1)))
    return packs


@pytest.mark.parametrize("n_batch", [12, 5200], ids=["small", "large"])
def test_lsop_handmade_containers(n_batch):
    """legacy (type 0, both header revisions, checksum on and off), Deflate (type 1) and canonical (type 2) containers around edge
    streams; a small batch (k_lsop_unpack2 from the first bit) and one of test_gpu_lsop_head's N_BATCH tiles (k_lsop_head's
    lane-per-tile threshold passed)"""
    import gridfour_amd
    nr, nc = 24, 40
    packs = _lsop_packs(nr, nc)
    want = [oracle.lsop12_decode(nr, nc, pk) for pk in packs]
    assert len(packs) == 12
    batch = [packs[t % len(packs)] for t in range(n_batch)]
    codec = gridfour_amd.LsCodecHip()
    vals, st = codec.decode_batch(nr, nc, batch)
    for t in range(len(batch)):
        assert st[t] == 0 and np.array_equal(vals[t], want[t % len(packs)]), (t, st[t])


# ---------------------------------------------------------------- the byte path at its row limit


def _limit_shapes():
    """the saturated tiles' shapes (value_edges.byte_path_limit_shapes), checked before any test runs: every build with every
    residue of nCols mod 4, the 256-thread build at RB = 255 rows per wave and one row more at RB = 256, the two other builds at the
    fused stage's ring limit for Differencing (so the shapes cannot drift to shorter tiles without this module failing)"""
    shapes = ve.byte_path_limit_shapes()
    for build in rp.BUILDS:
        mine = [(nr, nc) for b, nr, nc in shapes if b == build]
        assert sorted(nc % 4 for _, nc in mine) == [0, 1, 2, 3], (build, mine)
        waves = build // 64
        for nr, nc in mine:
            if build == 256:
                assert -(-nr // waves) == 255 and -(-(nr + 1) // waves) == 256, (nr, nc)
            else:
                assert ve.fused_ring(DIFF, nr, nc, build) and not ve.fused_ring(DIFF, nr + 1, nc, build), (build, nr, nc)
    return shapes


SATURATED = _limit_shapes()


@pytest.mark.parametrize("build,nr,nc", SATURATED, ids=["t%d-%dx%d" % s for s in SATURATED])
def test_byte_path_saturated_tiles(build, nr, nc):
    """all residuals +126 (the biased 16-bit column sums at their top) and all -126 (their bottom), Differencing, Linear and
    Triangle, at the tallest shape of the build whose Differencing tiles the byte path takes and one row more (the general value
    stage, or the general kernel where the fused stage has no ring).  The route report cannot tell the byte path from the general
    value stage inside the fast kernel: the restatements of byte_path_eligible and fused_plan say which one the tile takes, the
    retry word that the general kernel received exactly the tiles without a ring."""
    import gridfour_amd
    ctx = _ctx()
    codec = gridfour_amd.CodecHuffmanHip(context=ctx)
    for rows in (nr, nr + 1):
        p = rp.plan(KIND_HUFFMAN, rows, nc, 6)
        for model in MODELS:
            ring = ve.fused_ring(model, rows, nc, p.decThreads)
            eligible = ring and ve.byte_path_eligible(model, rows, nc, p.fastM32, p.decThreads)
            assert rows == nr + 1 or model != DIFF or eligible, (model, rows, nc)
            tiles, packs = [], []
            for value in (126, -126):
                v, res = ve.saturated_tile(model, rows, nc, value)
                res = res.astype(np.int64)
                res[-1] = value - np.sign(value)              # a second symbol: the text is not the single-symbol form
                tiles += [v, ve.tile_from_residuals(model, rows, nc, res, int(v[0]))[0]]
            for v in tiles:
                pk, used = oracle.codec_huffman_encode(0, rows, nc, v, predictor_mask=1 << (model - 1))
                assert used == model
                packs.append(pk)
            vals, st = codec.decode_batch(rows, nc, packs)
            ctx.synchronize()
            assert (st == 0).all(), (model, rows, st)
            for k, v in enumerate(tiles):
                bad = np.nonzero(vals[k] != v)[0]
                assert bad.size == 0, (model, rows, nc, k, bad.size, int(bad[0]) if bad.size else -1)
            rep = rp.report(ctx)
            assert rep.decBits & rp.dec_bit(rp.DEC_FAST, p.decThreads)
            assert rep.flags[_retry_word(p)] == (0 if ring else 1), (model, rows, nc, eligible, list(rep.flags))
