"""Every build and form of the Huffman and canonical paths, at shapes the route plan assigns to it, with the route proven.

The shapes come from the plan at run time (tests/route_plan.py: the first and the last square of an instantiation's domain within
the sweep, from 2x2 -- the reference declines or throws on single-row and single-column tiles of some codecs -- and capped in cells
where a GPU batch would be large), so an occupancy change that moves a shape to another build moves the test with it.  Every case is bit-exact against the oracle -- packings and decoded cells -- and asserts from the context's route
report (gf_internal_route_report) that the planned kernels launched and that the retry words are set or clear as the data
intends: did the general kernel, k_canon_decode or k_huffman_pack_rare receive a tile, and how many tiles did the pre-pass list
for the roomy run."""
import numpy as np
import pytest

import oracle
import route_plan as rp
from route_plan import KIND_CANON, KIND_HUFFMAN, KIND_RAW_M32
from tilegen import NULL, make_tile

pytestmark = pytest.mark.gpu
DOMAINS = rp.domains()


def _ctx():
    import gridfour_amd
    return gridfour_amd.GvrsHipContext(0)


def _ends(name, min_cells=1, max_cells=1 << 16):
    """first and last square of the instantiation's domain within the sweep, among squares of 2x2 and min_cells..max_cells cells"""
    return rp.square_ends(DOMAINS, name, min_cells, max_cells)


def _need(shape):
    assert shape is not None, "the route plan no longer gives this instantiation a shape of the sweep"
    return shape


def _cases(variant, mode, min_cells=1, max_cells=1 << 16):
    out = []
    for b in rp.BUILDS:
        for shape in _ends("%s:%s/%d" % (variant, rp.MODES[mode], b), min_cells, max_cells):
            out.append(pytest.param(b, shape, id="t%d-%s" % (b, "%dx%d" % shape if shape else "none")))
    return out


def _n_tiles(shape, want=6):
    return max(1, min(want, (1 << 19) // (shape[0] * shape[1])))


_device_roundtrip = rp.device_roundtrip


def _retry_word(p):
    """the decode retry word of a CodecHuffman batch: word 1 with a roomy budget, word 0 without"""
    return 1 if p.ldsM32Roomy else 0


_roomy_tiles = rp.roomy_tiles


def _max_stride(r, c):
    from gridfour_amd import _lib
    return int(_lib.lib().gf_huffman_max_packing(r, c))


# ---------------------------------------------------------------- k_huffman_decode, each build


@pytest.mark.parametrize("build,shape", _cases("huffman", rp.DEC_FAST, min_cells=1024))
def test_fast_decode_each_build(build, shape):
    """DEC_FAST on smooth terrain: the fast kernel of the planned build decodes every tile, the general one receives none
    (from 32x32 on: the fused stage of the fast kernel leaves some smaller shapes to the general kernel, fused_plan)"""
    r, c = _need(shape)
    ctx = _ctx()
    tiles = [make_tile("smooth", r, c, seed=s) for s in range(_n_tiles(shape))]
    _, enc, dec, p = _device_roundtrip(ctx, KIND_HUFFMAN, r, c, tiles)
    assert p.decThreads == build
    assert dec.decBits & rp.dec_bit(rp.DEC_FAST, build) and dec.decBits & rp.dec_bit(rp.DEC_GENERAL, build)
    assert dec.flags[_retry_word(p)] == 0, "the general kernel received a smooth tile"
    assert enc.encBits & rp.ENC_SPLIT and enc.flags[5] == 0, "k_huffman_pack_rare received a tile"


@pytest.mark.parametrize("build,shape", _cases("huffman", rp.DEC_GENERAL, min_cells=2048))
def test_general_decode_after_retry_each_build(build, shape):
    """DEC_GENERAL: 32-bit noise outgrows every LDS budget; the fast kernel leaves the tiles and the general kernel decodes them"""
    r, c = _need(shape)
    ctx = _ctx()
    tiles = [make_tile("noise32", r, c, seed=s) for s in range(_n_tiles(shape, 3))]
    tiles.append(make_tile("smooth", r, c, seed=9))
    _, _, dec, p = _device_roundtrip(ctx, KIND_HUFFMAN, r, c, tiles, slot_stride=_max_stride(r, c))
    assert p.decThreads == build
    assert dec.flags[_retry_word(p)] != 0, "no tile reached the general kernel"


@pytest.mark.parametrize("build,shape", _cases("huffman", rp.DEC_FAST_ROOMY, min_cells=6000))
def test_roomy_run_each_build(build, shape):
    """DEC_FAST_ROOMY: tiles between the fast run's buffer and the roomy one; the pre-pass lists them all, the general kernel
    receives none"""
    r, c = _need(shape)
    ctx = _ctx()
    n = _n_tiles(shape, 5)
    tiles = _roomy_tiles(r, c, n, 3, rp.plan(KIND_HUFFMAN, r, c, n + 1)) + [make_tile("smooth", r, c, seed=1)]
    b, _, dec, p = _device_roundtrip(ctx, KIND_HUFFMAN, r, c, tiles)
    assert p.decThreads == build and p.roomyForm == rp.ROOMY_BEHIND
    for t in range(n):
        n_m32 = int.from_bytes(b.get_packing(t, 10)[6:10], "little")
        assert p.fastM32 < n_m32 <= p.ldsM32Roomy, ("not a roomy tile", t, n_m32, p.fastM32, p.ldsM32Roomy)
    assert dec.decBits & rp.dec_bit(rp.DEC_FAST_ROOMY, build)
    assert dec.roomySeen - 1 == n, (dec.roomySeen, n)
    assert dec.flags[1] == 0, "a roomy tile reached the general kernel"


@pytest.mark.parametrize("build,shape", _cases("deflate", rp.DEC_GENERAL, max_cells=1 << 16))
def test_raw_m32_general_decode_each_build(build, shape):
    """DEC_GENERAL with raw M32 (CodecDeflate after inflate)"""
    import gridfour_amd
    r, c = _need(shape)
    ctx = _ctx()
    codec = gridfour_amd.CodecDeflateHip(context=ctx)
    tiles = np.stack([make_tile(k, r, c, seed=s) for s, k in enumerate(["smooth", "noise8", "sparse_big"])])
    packs, preds, st = codec.encode_batch(0, r, c, tiles)
    for t in range(len(tiles)):
        ref, used = oracle.codec_deflate_encode(0, r, c, tiles[t])
        assert st[t] == 0 and packs[t] == ref and preds[t] == used, t
    vals, st = codec.decode_batch(r, c, packs)
    ctx.synchronize()
    assert (st == 0).all() and np.array_equal(vals, tiles)
    rep = rp.report(ctx)
    p = rp.plan(KIND_RAW_M32, r, c, len(tiles))
    assert p.decThreads == build and rep.decKind == KIND_RAW_M32
    assert rep.decBits == p.decBits == rp.dec_bit(rp.DEC_GENERAL, build)


@pytest.mark.parametrize("build,shape", _cases("analyze", rp.DEC_ANALYZE, max_cells=1 << 16))
def test_analyze_each_build(build, shape):
    """DEC_ANALYZE: CodecHuffman.analyze sums against the oracle's decode, in each build (the 1024-thread one included)"""
    import gridfour_amd
    from test_gpu_analyze import _expected
    r, c = _need(shape)
    ctx = _ctx()
    codec = gridfour_amd.CodecHuffmanHip(context=ctx)
    kinds = ["smooth", "noise8", "steps", "uniform", "sparse_big", "ramp"]
    tiles = np.stack([make_tile(k, r, c, seed=s) for s, k in enumerate(kinds)])
    packs, preds, st = codec.encode_batch(0, r, c, tiles)
    packs = [pk for pk in packs if pk is not None]
    for t, pk in enumerate(packs):
        assert pk == oracle.codec_huffman_encode(0, r, c, tiles[t])[0], t
    codec.clearAnalysisData()
    status = codec.analyze_batch(r, c, packs)
    ctx.synchronize()
    assert (status == 0).all()
    rep = rp.report(ctx)
    p = rp.plan(KIND_HUFFMAN, r, c, len(packs), 0, 1)
    assert p.decThreads == build and rep.decBits == p.decBits and rep.decBits & rp.dec_bit(rp.DEC_ANALYZE, build)
    want, want_e = _expected(r, c, packs)
    got = codec.analysis_data()
    for k in range(6):
        have = [int(got[k][f]) for f in ("n_tiles", "n_bytes", "n_symbols", "n_bits_overhead", "n_m32_counted", "sum_length_m32",
                                         "sum_observed_m32")]
        assert have == list(want[k]), (k, have, list(want[k]))
        assert got[k]["sum_entropy_m32"] == pytest.approx(want_e[k], rel=1e-12, abs=1e-12)


# ---------------------------------------------------------------- the canonical decoder


def _with_nulls(r, c, seed):
    v = make_tile("smooth", r, c, seed=seed).copy()
    v[(r * c) // 3:(r * c) // 3 + max(1, (r * c) // 5)] = NULL
    return v


@pytest.mark.parametrize("build,shape", _cases("canon", rp.DEC_FAST_CANON))
def test_canon_fast_run_and_takeover_each_build(build, shape):
    """DEC_FAST_CANON: plain tiles in the fast run; tiles with null/escape symbols in the same batch go to k_canon_decode"""
    r, c = _need(shape)
    ctx = _ctx()
    n = _n_tiles(shape, 4)
    plain = [make_tile("smooth", r, c, seed=s) for s in range(n)]
    _, enc, dec, p = _device_roundtrip(ctx, KIND_CANON, r, c, plain)
    assert p.viaFast and p.decThreads == build and dec.decBits & rp.dec_bit(rp.DEC_FAST_CANON, build)
    assert enc.encBits & rp.CANON_ENC_1 and not enc.encBits & rp.CANON_ENC_0
    mixed = plain[:2] + [_with_nulls(r, c, 5), make_tile("noise32", r, c, seed=6)]
    _, _, dec, p = _device_roundtrip(ctx, KIND_CANON, r, c, mixed, slot_stride=_max_stride(r, c))
    assert dec.decBits & rp.dec_bit(rp.DEC_FAST_CANON, build)
    assert dec.flags[0] != 0, "no tile was left to k_canon_decode"


def _canon_edge_pair():
    """two shapes of 6,999 and 7,000 cells on which the plan picks the 256- and the 512-thread k_canon_decode"""
    for a, b in (((3, 2333), (70, 100)), ((1, 6999), (1, 7000)), ((6999, 1), (7000, 1))):
        if rp.plan(KIND_CANON, *a).canonThreads == 256 and rp.plan(KIND_CANON, *b).canonThreads == 512:
            return a, b
    raise AssertionError("no shape pair at 6,999 / 7,000 cells changes the k_canon_decode build")


@pytest.mark.parametrize("side", [0, 1])
def test_canon_decode_builds_at_7000_cells(side):
    shape = _canon_edge_pair()[side]
    r, c = _need(shape)
    ctx = _ctx()
    tiles = [_with_nulls(r, c, 1), make_tile("noise16", r, c, seed=2), make_tile("smooth", r, c, seed=3)]
    _, _, dec, p = _device_roundtrip(ctx, KIND_CANON, r, c, tiles)
    want = rp.CANON_DEC_T512 if side else rp.CANON_DEC_T256
    assert p.canonThreads == (512 if side else 256) and dec.decBits & want


@pytest.mark.parametrize("build,shape", [pytest.param(256, s, id="t256-%s" % ("%dx%d" % s if s else "none")) for s in _ends("canon:k_canon_decode/256")]
                         + [pytest.param(512, s, id="t512-%s" % ("%dx%d" % s if s else "none")) for s in _ends("canon:k_canon_decode/512")])
def test_canon_decode_domain_ends(build, shape):
    r, c = _need(shape)
    ctx = _ctx()
    tiles = [_with_nulls(r, c, 4), make_tile("sparse_big", r, c, seed=5), make_tile("extremes", r, c, seed=6)]
    _, _, dec, p = _device_roundtrip(ctx, KIND_CANON, r, c, tiles, slot_stride=_max_stride(r, c))
    assert p.canonThreads == build and dec.decBits & (rp.CANON_DEC_T512 if build == 512 else rp.CANON_DEC_T256)


# ---------------------------------------------------------------- the roomy run's three forms


def test_roomy_forms_beside_behind_skipped():
    """beside: 4,096 rough tiles on a fresh context; behind: a small batch after a rough one; skipped: a small batch after a smooth
    one (the hint says none) -- bit-exact on a sample, the roomy count and the retry words as the data intends"""
    r, c = 120, 150
    ctx = _ctx()
    _, _, dec, p = _device_roundtrip(ctx, KIND_HUFFMAN, r, c, style=oracle.DEM_STYLE_ROUGH, n_tiles=4096, sample=12)
    assert dec.roomyForm == rp.ROOMY_BESIDE and dec.prepass == 1
    assert dec.decBits & rp.dec_bit(rp.DEC_FAST_ROOMY, p.decThreads) and dec.roomySeen > 1, dec.roomySeen
    _, _, dec, p = _device_roundtrip(ctx, KIND_HUFFMAN, r, c, style=oracle.DEM_STYLE_ROUGH, n_tiles=1024, sample=8)
    assert dec.roomyForm == rp.ROOMY_BEHIND and dec.roomySeen > 1
    _, _, dec, p = _device_roundtrip(ctx, KIND_HUFFMAN, r, c, style=0, n_tiles=1024, sample=8)
    assert dec.roomyForm == rp.ROOMY_BEHIND and dec.roomySeen == 1          # (the hint came from the rough batch)
    _, _, dec, p = _device_roundtrip(ctx, KIND_HUFFMAN, r, c, style=0, n_tiles=1024, sample=8)
    assert dec.roomyForm == rp.ROOMY_SKIPPED and not dec.decBits & rp.dec_bit(rp.DEC_FAST_ROOMY, p.decThreads)
    assert dec.flags[1] == 0
    # a rough batch with the roomy run skipped: the first run and the general kernel take the listed tiles
    _, _, dec, p = _device_roundtrip(ctx, KIND_HUFFMAN, r, c, style=oracle.DEM_STYLE_ROUGH, n_tiles=1024, sample=8)
    assert dec.roomyForm == rp.ROOMY_SKIPPED and dec.roomySeen > 1


def test_large_rough_batch_wave_prepass():
    """k_huffman_parse_trees<64> (more than 4,096 tiles) with the roomy run beside"""
    ctx = _ctx()
    _, _, dec, p = _device_roundtrip(ctx, KIND_HUFFMAN, 120, 150, style=oracle.DEM_STYLE_ROUGH, n_tiles=4500, sample=10)
    assert dec.prepass == 64 and dec.decBits & rp.TREES_64 and dec.roomyForm == rp.ROOMY_BESIDE
    _, _, dec, p = _device_roundtrip(ctx, KIND_CANON, 120, 150, n_tiles=4500, style=0, sample=10)
    assert dec.decBits & rp.LENGTHS_64


# ---------------------------------------------------------------- the encoder's forms


def test_encoder_pack_rare_receives_long_code_tiles():
    """k_huffman_pack's bit window takes a step of 2,048 cells only while M32 bytes per value x the longest code stays under
    64 bits; tiles past that go to k_huffman_pack_rare (word 5 of the retry words counts them).  Geometric row differences give
    codes of 15 bits and more, two steps of 2^30 give five-byte values; the smooth tile beside them must not go there."""
    r, c = 120, 150
    ctx = _ctx()
    rng = np.random.default_rng(r + c)
    tiles = []
    for k in range(3):
        v = (rng.geometric(0.5, r * c) - 1).astype(np.int64).cumsum()
        v[(r * c) // 3 + k:] += 2 ** 30
        v[2 * (r * c) // 3 + k:] -= 2 ** 30
        tiles.append(v.astype(np.int32))
    tiles.append(make_tile("smooth", r, c, seed=2))
    _, enc, _, _ = _device_roundtrip(ctx, KIND_HUFFMAN, r, c, tiles, slot_stride=_max_stride(r, c))
    assert enc.encBits & rp.ENC_PACK_RARE and 1 <= enc.flags[5] < len(tiles), list(enc.flags)


def test_encoder_general_form_past_the_lean_limit():
    """k_huffman_encode<false>: tiles of 2^23 / 6 cells and more (first such shape of the sweep with two or more rows)"""
    shape = next(s for s in DOMAINS["huffman:k_huffman_encode<false>"] if s[0] >= 2)
    r, c = _need(shape)
    ctx = _ctx()
    _, enc, _, _ = _device_roundtrip(ctx, KIND_HUFFMAN, r, c, [make_tile("smooth", r, c, seed=1)])
    assert enc.encBits & rp.ENC_GENERAL and not enc.encBits & rp.ENC_SPLIT


@pytest.mark.parametrize("past", [0, 1])
def test_one_tile_path_at_the_lean_limit(past):
    """the one-tile path (replayed graph): the 1024-thread encoder at the largest lean shape, the general form one cell past it"""
    import gridfour_amd
    r = 2
    c = rp.LEAN_MAX_CELLS // 2 + past
    assert (6 * r * c < (1 << 23)) == (not past)
    ctx = _ctx()
    codec = gridfour_amd.CodecHuffmanHip(context=ctx)
    tile = np.random.default_rng(3).integers(-2, 3, r * c).astype(np.int32)     # (short codes: the lean packer keeps the tile)
    ref = oracle.codec_huffman_encode(0, r, c, tile)[0]
    assert codec.encode(0, r, c, tile) == ref                 # (the first call of a shape takes the batch path)
    assert codec.encode(0, r, c, tile) == ref                 # (the second one captures and replays the lean graph)
    ctx.synchronize()
    rep = rp.report(ctx)
    p = rp.plan(KIND_HUFFMAN, r, c, 1, lean=1)
    assert p.leanEncode == (not past) and rep.encBits == p.encBits, (hex(rep.encBits), hex(p.encBits))
    assert rep.encBits & (rp.ENC_GENERAL if past else rp.ENC_LEAN_T1024)


def test_one_tile_decode_path():
    """the one-tile decode path: DEC_FAST of the 1024-thread build alone"""
    import gridfour_amd
    r, c = 120, 150
    ctx = _ctx()
    codec = gridfour_amd.CodecHuffmanHip(context=ctx)
    tile = make_tile("smooth", r, c, seed=8)
    pk = oracle.codec_huffman_encode(0, r, c, tile)[0]
    for _ in range(3):
        assert np.array_equal(codec.decode(r, c, pk), tile)
    ctx.synchronize()
    rep = rp.report(ctx)
    p = rp.plan(KIND_HUFFMAN, r, c, 1, lean=1)
    assert rep.decBits == p.decBits == rp.TREES_1 | rp.dec_bit(rp.DEC_FAST, 1024)
