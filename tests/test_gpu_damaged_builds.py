"""Damaged packings through every production build of the Huffman and canonical decoders, held to the oracle's verdict.

The decode contract: where the oracle decodes a packing, the device returns status 0 and the same cells bit for bit;
where the oracle throws, the device returns GF_ERR_FORMAT or GF_ERR_BOUNDS -- never 0, never GF_ERR_UNSUPPORTED, never an internal
code.  The documented deviations (nM32 > 6 * cells, trees deeper than 63) are recognised by exact predicates (damage.deviation)
and must give an error.  The damage comes from tests/damage.py; its sets are pinned on the CPU by tests/test_damage_sets.py.

Shapes come from the route plan at run time, as in test_gpu_routes.py.  Every batch interleaves good tiles with the damaged
ones and runs twice through the device entry point -- packings in slots whose padding holds 0xA5, and packings compacted into
one blob at odd offsets, each truncated packing followed directly by its neighbour's bytes -- and, for CodecHuffman, once more
through the host-memory batch.  The cells and statuses go to buffers with a guard region behind the last tile, and the route
report must equal the plan."""
import numpy as np
import pytest

import damage as D
import oracle
import route_plan as rp
from route_plan import KIND_CANON, KIND_HUFFMAN, KIND_RAW_M32
from tilegen import NULL, make_tile

pytestmark = pytest.mark.gpu
DOMAINS = rp.domains()
GF_ERR_FORMAT, GF_ERR_BOUNDS = -1, -2
GUARD = 4096                                     # bytes behind the last tile's cells and status
SENTINEL = 0x5A
KIND = {D.HUFFMAN: KIND_HUFFMAN, D.CANON: KIND_CANON, D.DEFLATE: KIND_RAW_M32}
PREFIX = {D.HUFFMAN: "gf_huffman", D.CANON: "gf_canon", D.DEFLATE: "gf_deflate"}
_verdicts = {}


def _ctx():
    import gridfour_amd
    return gridfour_amd.GvrsHipContext(0)


def _shape(variant, name, build, **kw):
    """one plan-selected square of the build: the last of the 256-thread domain, the first of the others"""
    ends = rp.square_ends(DOMAINS, "%s:%s/%d" % (variant, name, build), **kw)
    assert ends[0] is not None, "the route plan no longer gives %s/%d a shape of the sweep" % (name, build)
    return ends[-1] if build == 256 else ends[0]


def _verdict(kind, r, c, pk):
    """the oracle's cells or None (thrown), once per distinct packing"""
    key = (kind, r, c, pk)
    if key not in _verdicts:
        _verdicts[key] = D.oracle_decode(kind, r, c, pk)
    return _verdicts[key]


def _encode(kind, r, c, v):
    f = {D.HUFFMAN: oracle.codec_huffman_encode, D.CANON: oracle.codec_canon_encode, D.DEFLATE: oracle.codec_deflate_encode}[kind]
    return f(0, r, c, v)[0]


def _dem(r, c, n, seed=7, style=0):
    return oracle.dem_tiles(oracle.DEM_SEED + seed, r, c, 144, 0, n, style=style).reshape(n, r * c)


def _nulls(r, c, seed):
    v = make_tile("smooth", r, c, seed=seed).copy()
    v[(r * c) // 3:(r * c) // 3 + max(1, (r * c) // 5)] = NULL
    return v


def _batch(goods, damaged, every=7):
    """good tiles between the damaged ones: items (label, packing, original cells)"""
    items, g = [], 0
    for k, (label, pk, orig) in enumerate(damaged):
        if k % every == 0:
            items.append(("good %d" % (g % len(goods)),) + goods[g % len(goods)])
            g += 1
        items.append((label, pk, orig))
    items.append(("good last",) + goods[-1])
    return items


def _damaged(kind, r, c, tiles, seed, parts=("header", "tree", "text", "length")):
    out, goods = [], []
    for k, v in enumerate(tiles):
        pk = _encode(kind, r, c, v)
        goods.append((pk, v))
        out += [(lab, p, v) for lab, p in D.damage_set(pk, kind, r, c, seed + k, parts)]
    return goods, out


def _dev_decode(ctx, kind, r, c, packs, compacted):
    """the device entry point on device buffers of the test's own: (cells, status, route report, plan)"""
    import gridfour_amd
    from gridfour_amd import _lib
    nt, cells = len(packs), r * c
    lens = np.array([len(p) for p in packs], np.uint32)
    if compacted:
        lead = 1                                 # every packing at an odd byte alignment or behind its neighbour's last byte
        offsets = np.zeros(nt + 1, np.uint64)
        offsets[0] = lead
        offsets[1:] = lead + np.cumsum(lens, dtype=np.uint64)
        blob = np.frombuffer(b"\xa5" * lead + b"".join(packs) + b"\xa5" * 67, np.uint8)
        stride = 0
    else:
        stride = (int(lens.max()) + 16 + 15) // 16 * 16
        blob = np.full(nt * stride + 64, 0xA5, np.uint8)
        for t, p in enumerate(packs):
            blob[t * stride:t * stride + len(p)] = np.frombuffer(p, np.uint8)
    B = gridfour_amd.DeviceBuffer
    d_blob = B(ctx, blob.nbytes).upload(blob)
    d_len = B(ctx, lens.nbytes).upload(lens)
    d_off = B(ctx, (nt + 1) * 8).upload(offsets) if compacted else None
    d_val = B(ctx, nt * cells * 4 + GUARD).fill(SENTINEL)
    d_st = B(ctx, nt * 4 + GUARD).fill(SENTINEL)
    ctx.synchronize()
    seen = rp.report(ctx).roomySeen              # the hint the decode's plan reads
    fn = getattr(_lib.lib(), PREFIX[kind] + "_decode_batch_i32_dev")
    _lib.check(fn(ctx.handle, None, r, c, nt, d_blob.ptr, blob.nbytes, d_off.ptr if compacted else None, stride, d_len.ptr,
                  d_val.ptr, d_st.ptr), PREFIX[kind] + "_decode_batch_i32_dev")
    ctx.synchronize()
    rep = rp.report(ctx)
    vals = d_val.download(np.int32, nt * cells).reshape(nt, cells)
    st = d_st.download(np.int32, nt)
    assert (d_val.download(np.uint8, GUARD, nt * cells * 4) == SENTINEL).all(), "cells written past the last tile"
    assert (d_st.download(np.uint8, GUARD, nt * 4) == SENTINEL).all(), "status written past the last tile"
    for b in (d_blob, d_len, d_off, d_val, d_st):
        if b is not None:
            b.free()
    p = rp.plan(KIND[kind], r, c, nt, 0, 0, seen)
    assert rep.decKind == KIND[kind]
    assert (rep.decBits, rep.prepass, rep.roomyForm) == (p.decBits, p.prepass, p.roomyForm), \
        (hex(rep.decBits), hex(p.decBits), rep.prepass, p.prepass, rep.roomyForm, p.roomyForm)
    return vals, st, rep, p


def _check(kind, r, c, items, vals, st, where):
    """the verdict rule for every tile; returns the verdicts seen and the count of accepted damage that changed the cells"""
    wrong, seen, changed = [], set(), 0
    for k, (label, pk, orig) in enumerate(items):
        s = int(st[k])
        dev = D.deviation(pk, kind, r * c)
        if dev is not None:
            if s not in (GF_ERR_FORMAT, GF_ERR_BOUNDS):
                wrong.append((k, label, s, "deviation: " + dev))
            continue
        want = _verdict(kind, r, c, pk)
        if want is None:
            seen.add("throws")
            if s not in (GF_ERR_FORMAT, GF_ERR_BOUNDS):
                wrong.append((k, label, s, "oracle throws"))
        else:
            seen.add("decodes")
            if s != 0 or not np.array_equal(vals[k], want):
                wrong.append((k, label, s, "oracle decodes"))
            elif not np.array_equal(want, orig):
                changed += 1
            if label.startswith("good") and not np.array_equal(want, orig):
                wrong.append((k, label, s, "good tile"))
    assert not wrong, (where, len(wrong), wrong[:10])
    return seen, changed


def _run(ctx, kind, r, c, items, host=True, check_sets=True):
    """both device forms (and the host batch for CodecHuffman); returns the last route report and plan"""
    import gridfour_amd
    packs = [pk for _, pk, _ in items]
    for compacted in (False, True):
        vals, st, rep, p = _dev_decode(ctx, kind, r, c, packs, compacted)
        seen, changed = _check(kind, r, c, items, vals, st, ("compacted" if compacted else "slots", r, c))
    if check_sets:
        assert seen == {"throws", "decodes"} and changed > 0, (seen, changed)
    if host and kind == D.HUFFMAN:
        vals, st = gridfour_amd.CodecHuffmanHip(context=ctx).decode_batch(r, c, packs)
        _check(kind, r, c, items, vals, st, ("host", r, c))
    return rep, p


# ---------------------------------------------------------------- CodecHuffman, k_huffman_decode<DEC_FAST> per build


def _fast_shapes():
    out = []
    for b in rp.BUILDS:
        s = _shape("huffman", rp.MODES[rp.DEC_FAST], b, min_cells=1024)
        out.append(pytest.param(b, s, id="t%d-%dx%d" % ((b,) + s)))
    for s in ((120, 150), (200, 200)):
        out.append(pytest.param(rp.plan(KIND_HUFFMAN, *s).decThreads, s, id="%dx%d" % s))
    return out


@pytest.mark.parametrize("build,shape", _fast_shapes())
def test_huffman_fast_each_build(build, shape):
    r, c = shape
    ctx = _ctx()
    smooth, dem, nul = make_tile("smooth", r, c, seed=1), _dem(r, c, 1)[0], _nulls(r, c, 2)
    goods, dmg = _damaged(D.HUFFMAN, r, c, [smooth], 11)
    g2, d2 = _damaged(D.HUFFMAN, r, c, [dem, nul], 12, parts=("header", "text", "length"))
    good, crafted = D.crafted_m32(D.HUFFMAN, r, c, smooth, 13)
    assert crafted[0][1] == good
    items = _batch(goods + g2, dmg + d2 + [(lab, pk, smooth) for lab, pk in crafted])
    rep, p = _run(ctx, D.HUFFMAN, r, c, items)
    assert p.decThreads == build and rep.decBits & rp.dec_bit(rp.DEC_FAST, build)


# ---------------------------------------------------------------- the roomy run, both forms


@pytest.mark.parametrize("build", [512, 1024])
def test_huffman_roomy_behind(build):
    r, c = _shape("huffman", rp.MODES[rp.DEC_FAST_ROOMY], build, min_cells=6000)
    ctx = _ctx()
    tiles = rp.roomy_tiles(r, c, 2, 5, rp.plan(KIND_HUFFMAN, r, c, 64))
    goods, dmg = _damaged(D.HUFFMAN, r, c, tiles[:1], 21, parts=("header", "text", "length"))
    g2, d2 = _damaged(D.HUFFMAN, r, c, tiles[1:], 22, parts=("tree",))
    rep, p = _run(ctx, D.HUFFMAN, r, c, _batch(goods + g2 + [(_encode(D.HUFFMAN, r, c, make_tile("smooth", r, c)),
                                                               make_tile("smooth", r, c))], dmg + d2[::3]))
    assert p.decThreads == build and p.roomyForm == rp.ROOMY_BEHIND and rep.roomySeen > 1


def test_huffman_beside_and_wave_prepass():
    """more than 4,096 tiles of 120 x 150 after a rough batch: the roomy run beside the first run, k_huffman_parse_trees<64>
    on damaged trees (smooth and roomy tiles)"""
    r, c = 120, 150
    ctx = _ctx()
    p = rp.plan(KIND_HUFFMAN, r, c, 64)
    roomy = rp.roomy_tiles(r, c, 2, 9, p)
    smooth = make_tile("smooth", r, c, seed=3)
    goods, dmg = _damaged(D.HUFFMAN, r, c, [smooth, roomy[0]], 31, parts=("tree",))
    g_roomy = (_encode(D.HUFFMAN, r, c, roomy[1]), roomy[1])
    _run(ctx, D.HUFFMAN, r, c, _batch([g_roomy], dmg[:40]), host=False)            # (sets the hint: roomy tiles seen)
    items = _batch(goods + [g_roomy], dmg)
    while len(items) < 4160:
        items.append(("good fill",) + (goods + [g_roomy])[len(items) % 3])
    rep, p = _run(ctx, D.HUFFMAN, r, c, items, host=False)
    assert len(items) > 4096 and rep.prepass == 64 and rep.decBits & rp.TREES_64 and rep.roomyForm == rp.ROOMY_BESIDE


# ---------------------------------------------------------------- DEC_GENERAL


@pytest.mark.parametrize("build", rp.BUILDS)
def test_huffman_general_each_build(build):
    r, c = _shape("huffman", rp.MODES[rp.DEC_GENERAL], build, min_cells=2048)
    ctx = _ctx()
    goods, dmg = _damaged(D.HUFFMAN, r, c, [make_tile("noise32", r, c, seed=4)], 41, parts=("header", "text", "length"))
    g2, d2 = _damaged(D.HUFFMAN, r, c, [make_tile("noise32", r, c, seed=5)], 42, parts=("tree",))
    rep, p = _run(ctx, D.HUFFMAN, r, c, _batch(goods + g2, dmg + d2[::4]))
    assert p.decThreads == build and rep.decBits & rp.dec_bit(rp.DEC_GENERAL, build)
    assert rep.flags[1 if p.ldsM32Roomy else 0] != 0, "no tile reached the general kernel"


# ---------------------------------------------------------------- CodecCanonHuffman


@pytest.mark.parametrize("build", rp.BUILDS)
def test_canon_fast_run_each_build(build):
    r, c = _shape("canon", rp.MODES[rp.DEC_FAST_CANON], build)
    ctx = _ctx()
    goods, dmg = _damaged(D.CANON, r, c, [make_tile("smooth", r, c, seed=6)], 51)
    g2, d2 = _damaged(D.CANON, r, c, [_nulls(r, c, 7), make_tile("sparse_big", r, c, seed=8)], 52, parts=("header", "text", "length"))
    rep, p = _run(ctx, D.CANON, r, c, _batch(goods + g2, dmg + d2))
    assert p.viaFast and p.decThreads == build and rep.decBits & rp.dec_bit(rp.DEC_FAST_CANON, build)
    assert rep.flags[0] != 0, "no tile was left to k_canon_decode"


@pytest.mark.parametrize("build", [256, 512])
def test_canon_decode_each_build(build):
    r, c = rp.square_ends(DOMAINS, "canon:k_canon_decode/%d" % build, min_cells=1024)[0 if build == 512 else -1]
    ctx = _ctx()
    goods, dmg = _damaged(D.CANON, r, c, [_nulls(r, c, 9)], 61)
    g2, d2 = _damaged(D.CANON, r, c, [make_tile("noise16", r, c, seed=10)], 62, parts=("header", "text", "length"))
    rep, p = _run(ctx, D.CANON, r, c, _batch(goods + g2, dmg + d2))
    assert p.canonThreads == build and rep.decBits & (rp.CANON_DEC_T512 if build == 512 else rp.CANON_DEC_T256)


def test_canon_wave_prepass():
    """more than 4,096 tiles of 120 x 150: k_canon_parse_lengths<64> on damaged length tables"""
    r, c = 120, 150
    ctx = _ctx()
    goods, dmg = _damaged(D.CANON, r, c, [make_tile("smooth", r, c, seed=12), _nulls(r, c, 13)], 71, parts=("tree",))
    items = _batch(goods, dmg)
    while len(items) < 4160:
        items.append(("good fill",) + goods[len(items) % 2])
    rep, p = _run(ctx, D.CANON, r, c, items)
    assert rep.prepass == 64 and rep.decBits & rp.LENGTHS_64


# ---------------------------------------------------------------- raw M32 (CodecDeflate)


@pytest.mark.parametrize("build", rp.BUILDS)
def test_raw_m32_crafted_each_build(build):
    r, c = _shape("deflate", rp.MODES[rp.DEC_GENERAL], build, min_cells=1024)
    ctx = _ctx()
    items = []
    for k, v in enumerate([make_tile("smooth", r, c, seed=14), _nulls(r, c, 15)]):
        good, crafted = D.crafted_m32(D.DEFLATE, r, c, v, 80 + k)
        assert crafted[0][1] == good
        items += [(lab, pk, v) for lab, pk in crafted]
    rep, p = _run(ctx, D.DEFLATE, r, c, items)
    assert p.decThreads == build and rep.decBits == rp.dec_bit(rp.DEC_GENERAL, build)


# ---------------------------------------------------------------- the one-tile path (replayed graph)


@pytest.mark.parametrize("shape", [(120, 150), (200, 200)])
def test_one_tile_path(shape):
    import gridfour_amd
    r, c = shape
    ctx = _ctx()
    codec = gridfour_amd.CodecHuffmanHip(context=ctx)
    v = make_tile("smooth", r, c, seed=16)
    good = _encode(D.HUFFMAN, r, c, v)
    dmg = D.damage_set(good, D.HUFFMAN, r, c, 91)
    _, crafted = D.crafted_m32(D.HUFFMAN, r, c, v, 92)
    picks = dmg[::max(1, len(dmg) // 24)] + crafted[1:]
    for _ in range(2):
        assert np.array_equal(codec.decode(r, c, good), v)
    wrong, seen = [], set()
    for label, pk in picks + [("good", good)]:
        try:
            got, err = codec.decode(r, c, pk), None
        except IOError as e:
            got, err = None, e
        dev = D.deviation(pk, D.HUFFMAN, r * c)
        want = None if dev else _verdict(D.HUFFMAN, r, c, pk)
        seen.add("throws" if want is None and not dev else "decodes" if want is not None else "deviation")
        if want is None:
            if err is None:
                wrong.append((label, "decoded where the oracle throws" if not dev else dev))
        elif got is None or not np.array_equal(got, want):
            wrong.append((label, "oracle decodes", str(err)))
    assert not wrong, wrong
    assert {"throws", "decodes"} <= seen
    ctx.synchronize()
    rep = rp.report(ctx)
    assert rep.decBits == rp.plan(KIND_HUFFMAN, r, c, 1, lean=1).decBits
