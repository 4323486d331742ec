"""tests/value_edges.py reaches every edge it claims to (CPU, the oracle only): every tile it builds has exactly the intended residual
stream, the M32 edge set holds both ends of every length with both signs, the canonical one both ends of every kind and of the
gap, and the oracle's codecs give each tile back -- the GPU tests of tests/test_gpu_value_edges.py cannot drift into testing
something easier without one of these failing."""
import numpy as np
import pytest

import oracle
import value_edges as ve
from oracle import canon_ref as R
from value_edges import DIFF, GAP, IMAX, LINEAR, NULL, NULLS, TRIANGLE

SHAPES = [(24, 40), (7, 13), (2, 5)]


def _same_stream(model, nr, nc, v, res):
    got, _ = oracle.predictor_encode_int(model, nr, nc, v)
    assert got is not None and np.array_equal(got, res), (model, nr, nc)


def test_m32_lengths_at_both_ends_with_both_signs():
    """the restated lengths agree with the oracle's CodecM32, and every length 1-6 appears at its lowest and highest |v|"""
    for v in ve.M32_EDGES:
        assert len(oracle.m32_encode(v)) == ve.m32_len(v), v
        got, n = oracle.m32_decode_seq(oracle.m32_encode(v), 1)
        assert got[0] == v and n == ve.m32_len(v), v
    want = {1: (0, 126), 2: (127, 254), 3: (255, 16638), 4: (16639, 2113790), 5: (2113791, 270549246), 6: (270549247, IMAX)}
    for n, (lo, hi) in want.items():
        for s in (1, -1):
            for a in (lo, hi):
                if a == 0:
                    continue
                assert s * a in ve.M32_EDGES and len(oracle.m32_encode(s * a)) == n, (n, s * a)
    assert -128 in ve.M32_EDGES and oracle.m32_encode(-127) == b"\x81\x00" and oracle.m32_encode(-128) == b"\x81\x01"
    assert NULL in ve.M32_EDGES and oracle.m32_encode(NULL) == b"\x80"
    assert -IMAX in ve.M32_EDGES and len(oracle.m32_encode(-IMAX)) == 6


def _java_count_kind(v):
    """the branch of countSymbols (oracle/canon_ref.py, CanonicalHuffman.java:352-418) a value takes, read off its node counts"""
    enc = R.CanonicalHuffman()
    enc.countSymbols(1, 0, [int(v)])
    esc2, esc8, nul = enc.symbolNodes[R.I_ESCAPE_2BITS].count, enc.symbolNodes[R.I_ESCAPE_1BYTE].count, enc.symbolNodes[R.I_NULL_DATA_CODE].count
    targets = [i for i in range(256) if enc.symbolNodes[i].count]
    kind = 7 if nul else (esc2 if esc2 else (3 + esc8 if esc8 else 0))
    return kind, (targets[0] if targets else 256)


def test_canonical_kinds_at_both_ends():
    """every kind 0-7 at its lowest and highest value and one past each, target symbols 0 and 255 in every kind, both ends of the
    gap -- against the Python restatement of countSymbols and the emit side of encode (:258 tests -8,333,608)"""
    for v in ve.CANON_EDGES:
        assert _java_count_kind(v) == (ve.canon_kind(v), ve.canon_target(v)), v
    bounds = [(-128, 127)] + [(lo, hi) for _, lo, hi in ve.CANON_KIND_RANGES[1:]] + [(-IMAX, IMAX)]
    for k in range(1, 7):
        lo, hi = bounds[k]
        inner_lo, inner_hi = bounds[k - 1]
        for v in (lo, hi, inner_lo - 1, inner_hi + 1):
            assert v in ve.CANON_EDGES and ve.canon_kind(v) == k, (k, v)
        assert k == 6 or (lo - 1 in ve.CANON_EDGES and hi + 1 in ve.CANON_EDGES)
        assert ve.canon_target(lo) == 0 and ve.canon_target(hi) == 255, k
    assert ve.canon_kind(-128) == 0 and ve.canon_target(-128) == 0 and ve.canon_target(127) == 255
    assert ve.canon_kind(NULL) == 7 and NULL in ve.CANON_EDGES
    for v in GAP:
        assert v in ve.CANON_EDGES and ve.canon_kind(v) == 5 and ve.canon_emit_kind(v) == 6
    assert ve.canon_emit_kind(GAP[1] + 1) == 5 and ve.canon_target(GAP[1] + 1) == 0
    assert ve.canon_emit_kind(GAP[0] - 1) == 6


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", [DIFF, LINEAR, TRIANGLE])
def test_value_tiles_carry_the_intended_stream(model, shape):
    nr, nc = shape
    pl = ve.placements(model, nr, nc)
    for r, c in ((0, 1), (1, 0), (nr - 1, nc - 1), (nr // 2, nc // 2)):
        p = ve.stream_index(model, nr, nc, r, c)
        res = np.zeros(ve.n_residuals(model, nr, nc), np.int64)
        res[p] = 12345
        v, _ = ve.tile_from_residuals(model, nr, nc, res, 7)
        got, _ = oracle.predictor_encode_int(model, nr, nc, v)
        assert np.nonzero(got)[0].tolist() == [p], (model, r, c)
    assert pl["last"] == ve.n_residuals(model, nr, nc) - 1
    for edges in (ve.M32_EDGES, ve.CANON_EDGES):
        for v, res in ve.value_tiles(model, nr, nc, edges):
            _same_stream(model, nr, nc, v, res)
            assert not (v == NULL).any()


def test_every_edge_reaches_every_placement():
    nr, nc = SHAPES[0]
    for model in (DIFF, LINEAR, TRIANGLE):
        pos = sorted(set(ve.placements(model, nr, nc).values()))
        for edges in (ve.M32_EDGES, ve.CANON_EDGES):
            tiles = ve.value_tiles(model, nr, nc, edges)
            for e, (v, res) in zip(edges, tiles):
                assert all(res[p] == e for p in pos), (model, e)


def test_phase_tiles_start_wide_values_at_every_byte_phase():
    nr, nc = SHAPES[0]
    for model in (DIFF, LINEAR, TRIANGLE):
        seen = set()
        ends = set()
        for v, res, pos in ve.phase_tiles(model, nr, nc):
            _same_stream(model, nr, nc, v, res)
            off = len(oracle.m32_encode_seq(res[:pos]))
            n = ve.m32_len(res[pos])
            seen.add((n, off % 4))
            m32 = oracle.m32_encode_seq(res)
            if pos == len(res) - 1:
                assert off + n == len(m32) and n == 6
                ends.add("last")
            if pos == 0:
                assert n == 6
                ends.add("first")
        assert seen >= {(n, ph) for n in range(2, 7) for ph in range(4)}, sorted(seen)
        assert ends == {"first", "last"}


def test_int_min_residuals_in_models_1_to_3():
    nr, nc = SHAPES[0]
    for model, v, res in ve.int_min_tiles(nr, nc):
        _same_stream(model, nr, nc, v, res)
        assert (res == NULL).sum() >= 4 and not (v == NULL).any()
        pk, used = oracle.codec_huffman_encode(0, nr, nc, v, predictor_mask=1 << (model - 1))
        assert used == model and np.array_equal(oracle.codec_huffman_decode(nr, nc, pk), v)


def test_nulls_tiles():
    for nr, nc in ((24, 40), (9, 11)):
        v, res = ve.nulls_tile(nr, nc, ve.M32_EDGES)
        _same_stream(NULLS, nr, nc, v, res)
        wide = {int(x) for x in res if x != NULL}
        assert (res == NULL).any() and len(wide & set(ve.WIDE)) >= 4, sorted(wide & set(ve.WIDE))
        pk, used = oracle.codec_huffman_encode(0, nr, nc, v)
        assert used == NULLS and np.array_equal(oracle.codec_huffman_decode(nr, nc, pk), v)


def test_densities_land_where_they_should():
    import route_plan as rp
    nr, nc = 120, 150
    p = rp.plan(rp.KIND_HUFFMAN, nr, nc, 4)
    assert p.ldsM32Roomy > p.fastM32
    for v, res in ve.roomy_edge_tiles(DIFF, nr, nc, 2, p):
        _same_stream(DIFF, nr, nc, v, res)
        assert p.fastM32 < ve.m32_bytes(DIFF, res) <= p.ldsM32Roomy
    v, res = ve.general_edge_tile(TRIANGLE, nr, nc)
    _same_stream(TRIANGLE, nr, nc, v, res)
    assert ve.m32_bytes(TRIANGLE, res) > max(p.ldsM32Roomy, 4 * nr * nc)
    v, res = ve.rare_edge_tile(nr, nc)
    _same_stream(DIFF, nr, nc, v, res)
    cl = oracle.huffman_encode(np.frombuffer(oracle.m32_encode_seq(res), np.uint8))[2]
    assert cl.max() >= 11 and max(ve.m32_len(x) for x in res) == 6


@pytest.mark.parametrize("model", [DIFF, LINEAR, TRIANGLE])
def test_saturated_tiles(model):
    for nc in (4, 5, 6, 7):
        for value in (126, -126):
            v, res = ve.saturated_tile(model, 40, nc, value)
            _same_stream(model, 40, nc, v, res)
            assert (res == value).all()


def test_oracle_roundtrips_every_tile():
    """oracle encode then decode gives every tile back, in CodecHuffman, CodecDeflate and CodecCanonHuffman; a canonical packing
    that holds a gap value is one the reference cannot read back (the oracle's decode raises)"""
    nr, nc = SHAPES[0]
    gap_fail = 0
    for model in (DIFF, LINEAR, TRIANGLE):
        mask = 1 << (model - 1)
        for v, _ in ve.value_tiles(model, nr, nc, ve.M32_EDGES):
            pk, used = oracle.codec_huffman_encode(0, nr, nc, v, predictor_mask=mask)
            assert used == model and np.array_equal(oracle.codec_huffman_decode(nr, nc, pk), v)
        for e, (v, _) in zip(ve.CANON_EDGES, ve.value_tiles(model, nr, nc, ve.CANON_EDGES)):
            pk, used = oracle.codec_canon_encode(0, nr, nc, v, predictor_mask=mask)
            assert used == model
            assert np.array_equal(oracle.codec_canon_decode(nr, nc, pk), v), e
        # the gap: read back where the background holds -1 (symbol 127 has a code), refused where it does not
        for v, res, minus_one in ve.gap_tiles(model, nr, nc):
            _same_stream(model, nr, nc, v, res)
            assert ((res == -1).any() == minus_one) and (res == GAP[0]).any() != (res == GAP[1]).any()
            pk, used = oracle.codec_canon_encode(0, nr, nc, v, predictor_mask=mask)
            assert used == model
            if minus_one:
                assert np.array_equal(oracle.codec_canon_decode(nr, nc, pk), v)
            else:
                with pytest.raises(IOError):
                    oracle.codec_canon_decode(nr, nc, pk)
                gap_fail += 1
    assert gap_fail == 6
    for v, _ in ve.value_tiles(DIFF, nr, nc, ve.M32_EDGES[:8]):
        pk, _ = oracle.codec_deflate_encode(0, nr, nc, v)
        assert np.array_equal(oracle.codec_deflate_decode(nr, nc, pk), v)


def test_nulls_sum_streams():
    """the hand-made DifferencingWithNulls streams put sums of Integer.MIN_VALUE next to edge values, and the three containers around
    one stream decode alike in the oracle"""
    r, c = 16, 24
    for k in range(3):
        sd, res, sums = ve.nulls_sum_stream(r, c, ve.M32_EDGES[k:] + ve.M32_EDGES[:k], seed=5 + 1000 * k, rng_seed=k)
        deflate, huffman, raw = ve.nulls_sum_packings(r, c, sd, res)
        want = oracle.codec_deflate_decode(r, c, deflate)
        assert np.array_equal(oracle.codec_huffman_decode(r, c, huffman), want)
        assert raw[:10] == deflate[:10] and oracle.m32_decode_seq(raw[10:], r * c)[0] == [int(x) for x in res]
        assert len(sums) >= r and all(want[i] == NULL and res[i] != NULL for i in sums)
        wide = {int(res[i - 1]) for i in sums if i % c} | {int(res[i + 1]) for i in sums if (i + 1) % c}
        assert len(wide & set(ve.WIDE)) >= 4, sorted(wide)


def test_byte_path_limit_shapes():
    """every k_huffman_decode build has a saturated-tile shape for each residue of nCols mod 4; the 256-thread build's stop at
    RB = 255 rows per wave (one row more: 256), the other builds' at the fused stage's ring limit for Differencing"""
    import route_plan as rp
    shapes = ve.byte_path_limit_shapes()
    for build in rp.BUILDS:
        mine = [(nr, nc) for b, nr, nc in shapes if b == build]
        assert sorted(nc % 4 for _, nc in mine) == [0, 1, 2, 3], (build, mine)
        for nr, nc in mine:
            p = rp.plan(rp.KIND_HUFFMAN, nr, nc, 4)
            assert p.decThreads == build and ve.byte_path_eligible(DIFF, nr, nc, p.fastM32, build) and ve.fused_ring(DIFF, nr, nc, build)
            if build == 256:
                assert -(-nr // 4) == 255 and -(-(nr + 1) // 4) == 256, (nr, nc)
            else:
                assert not ve.fused_ring(DIFF, nr + 1, nc, build), (build, nr, nc)


def test_lsop_containers():
    """the hand-made Deflate and canonical containers carry the two streams they were built around (read back from where the
    layout puts them), and the oracle's LSOP12 decode of each is the tile those streams make (tests/lsop_ref.py: with zero
    coefficients every interior prediction is 0)"""
    import struct
    import zlib

    import lsop_ref
    nr, nc = 24, 40
    coefs = np.zeros(12, np.float32)
    for k, edges in enumerate((ve.M32_EDGES, ve.CANON_EDGES)):
        init, inter = ve.lsop_streams(nr, nc, [e for e in edges if not ve.in_gap(e)], k)
        assert len(init) == ve.lsop_n_init(nr, nc) and len(inter) == ve.lsop_n_interior(nr, nc)
        i32 = lambda a: [int(x) for x in np.asarray(a, np.int64).astype(np.int32)]
        want = lsop_ref.reconstruct(nr, nc, 9, i32(init), i32(inter), coefs)
        for checksum in (False, True):
            pk = ve.lsop_deflate_container(9, coefs, init, inter, checksum)
            assert pk[1] == 1 | 0x40 | (0x80 if checksum else 0) and struct.unpack_from("<i", pk, 3)[0] == 9
            n_init, n_int = struct.unpack_from("<ii", pk, 55)          # behind codec, type, 12, seed, 12 floats
            z = zlib.decompressobj()
            m_init = z.decompress(pk[63 + 4 * checksum:])
            m_int = zlib.decompress(z.unused_data)
            assert len(m_init) == n_init and len(m_int) == n_int
            assert oracle.m32_decode_seq(m_init, len(init))[0] == i32(init)
            assert oracle.m32_decode_seq(m_int, len(inter))[0] == i32(inter)
            assert np.array_equal(oracle.lsop12_decode(nr, nc, pk), want)
            pk = ve.lsop_canon_container(9, coefs, init, inter, checksum)
            assert pk[1] == 2 | 0x40 | (0x80 if checksum else 0)
            got, pos = oracle.canon_decode(pk, len(init), 8 * (55 + 4 * checksum))
            assert got.tolist() == i32(init)
            got, _ = oracle.canon_decode(pk, len(inter), pos)
            assert got.tolist() == i32(inter)
            assert np.array_equal(oracle.lsop12_decode(nr, nc, pk), want)
