"""CPU-only: the Python restatement of LSOP08 (tests/lsop08_ref.py) holds together -- it round-trips, its LU agrees with an exact
rational solve, its rounding is told apart from LSOP12's, its numpy forms give the scalar forms' bits -- and what of the gf_lsop08_*
family can be checked without a device: the size functions, the argument refusals, the Java adapter and its shim kind (as text).
Then the tiles of tests/lsop08_cases.py: each has the property the GPU tests use it for."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest

import lsop08_cases as K
import lsop08_ref as R
import oracle
from gvrs_walk import tile_packings
from tilegen import make_tile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BOTH_TYPES = [(4, 4), (4, 5), (5, 4), (7, 9), (16, 16), (33, 65), (65, 66)]
DEFLATE_ONLY = [(66, 5), (5, 66), (129, 4), (4, 129)]


def _tiles(nr, nc):
    out = [("terrain0", R.terrain(nr, nc, 0)), ("terrain1", R.terrain(nr, nc, 1)), ("smooth", make_tile("smooth", nr, nc))]
    if nr * nc <= 33 * 65:
        out += [(k, make_tile(k, nr, nc)) for k in ("noise8", "noise32", "sparse_big")]
    return out


@pytest.mark.parametrize("shape", BOTH_TYPES + DEFLATE_ONLY, ids=lambda s: "%dx%d" % s)
def test_round_trip_counts_and_header(shape):
    nr, nc = shape
    done = 0
    for name, v in _tiles(nr, nc):
        pr = R.predict(nr, nc, v)
        if pr is None:
            assert R.encode(5, nr, nc, v) == (None, None)
            continue
        seed, u, init, inter = pr
        assert seed == int(v[0]) and len(init) == 2 * nc + 2 * nr - 5 and len(inter) == (nr - 2) * (nc - 2)
        assert np.array_equal(R.reconstruct(nr, nc, seed, init, inter, u), v), name
        chosen, ctype = R.encode(5, nr, nc, v)
        packs = {t: R.encode(5, nr, nc, v, force_type=t)[0] for t in (0, 1)}
        assert chosen == packs[ctype]
        # the choice: Huffman only where its body is strictly shorter
        assert (ctype == 0) == (len(packs[0]) < len(packs[1])), name
        m_init, m_int = oracle.m32_encode_seq(init), oracle.m32_encode_seq(inter)
        for t, p in packs.items():
            assert p[:3] == bytes([5, 0x40 | t, 8]) and p[3:7] == struct.pack("<i", seed) and p[7:39] == u.astype("<f4").tobytes()
            assert struct.unpack_from("<ii", p, 39) == (len(m_init), len(m_int)) and R.parse_header(p)[5] == 47
            assert np.array_equal(R.decode(nr, nc, p), v), (name, t)
            assert np.array_equal(R.decode(nr, nc, R.to_legacy_header(p)), v), (name, t)
            assert np.array_equal(R.decode(nr, nc, R.with_checksum_flag(p)), v), (name, t)
        done += 1
    assert done >= 2


def test_both_container_types_occur():
    assert R.encode(0, 33, 65, R.terrain(33, 65, 0))[1] == 0 and R.encode(0, 33, 65, R.terrain(33, 65, 1))[1] == 1
    assert R.encode(0, 64, 64, R.terrain(64, 64, 0))[1] == 0 and R.encode(0, 64, 64, make_tile("noise8", 64, 64))[1] == 1


@pytest.mark.parametrize("shape", [(3, 9), (9, 3)], ids=lambda s: "%dx%d" % s)
def test_small_tiles_decline(shape):
    nr, nc = shape
    assert R.predict(nr, nc, R.terrain(nr, nc)) is None and R.encode(0, nr, nc, R.terrain(nr, nc)) == (None, None)


def test_singular_tiles_decline():
    for nr, nc in ((4, 4), (16, 16), (33, 65)):
        assert R.predict(nr, nc, make_tile("uniform", nr, nc)) is None
        assert R.predict(nr, nc, make_tile("extremes", nr, nc)) is None


def test_single_symbol_segment():
    """A stream of one repeated byte takes HuffmanEncoder's 17-bit form (HuffmanEncoder.java:147-157): a 4 x 4 tile has four interior
    values, and a tile that is linear in the interior has four zeros there."""
    body = R.huffman_body(bytes([3, 3, 3]), bytes([0, 0, 0, 0]))
    assert len(body) == (17 + 17 + 7) // 8
    a, pos = oracle.huffman_decode(body, 3, 0)
    b, pos = oracle.huffman_decode(body, 4, pos)
    assert (a, b, pos) == (bytes([3, 3, 3]), bytes(4), 34)


def test_numpy_sums_are_the_scan_order_sums():
    for v, nr, nc in ((R.terrain(16, 16), 16, 16), (make_tile("noise32", 16, 16), 16, 16), (make_tile("sparse_big", 7, 9), 7, 9)):
        assert R.gram(nr, nc, v) == R.gram_fast(nr, nc, v)


def test_numpy_interior_is_the_scalar_interior():
    """interior_fast against interior(): every coefficient set of COEF_SETS (Inf, NaN, saturation at both limits, the half-way cases
    of p + 0.5f, negative predictions) on a smooth tile and on 32-bit noise, and each tile's own coefficients"""
    tiles = [(16, 16, R.terrain(16, 16)), (9, 11, make_tile("noise32", 9, 11)), (7, 70, make_tile("smooth", 7, 70)),
             (12, 9, np.random.default_rng(8).integers(-2 ** 31, 2 ** 31, 108).astype(np.int32))]
    for nr, nc, v in tiles:
        sets = dict(R.COEF_SETS, own=R.coefficients(nr, nc, v))
        for name, u in sets.items():
            tr = []
            slow = R.interior(nr, nc, v, u, trace=tr)
            assert slow == R.interior_fast(nr, nc, v, u), (nr, nc, name)
        assert len(slow) == R.n_interior(nr, nc)
    # ... and the sets still reach the edges they are there for, on the tile the comparison ran on
    v = tiles[1][2]
    with np.errstate(all="ignore"):
        tr = []
        R.interior(9, 11, v, R.COEF_SETS["inf_pair"], trace=tr)
        assert np.isnan(np.array(tr, np.float32)).any()
        tr = []
        R.interior(9, 11, v, R.COEF_SETS["sat_pos"], trace=tr)
        assert (np.array(tr, np.float32) > 3e9).any() and (np.array(tr, np.float32) < -3e9).any()


def test_container_from_streams_round_trips():
    """container() is what encode() writes, and a packing built from arbitrary streams and coefficients decodes to what
    reconstruct() makes of them, in both types"""
    nr, nc = 7, 9
    v = R.terrain(nr, nc, 0)
    seed, u, init, inter = R.predict(nr, nc, v)
    for t in (None, 0, 1):
        assert R.container(5, seed, u, init, inter, t) == R.encode(5, nr, nc, v, force_type=t)
    rng = np.random.default_rng(4)
    init = rng.integers(-2 ** 31, 2 ** 31, R.n_init(nr, nc)).tolist()
    inter = rng.integers(-70000, 70000, R.n_interior(nr, nc)).tolist()
    want = R.reconstruct(nr, nc, -12345, init, inter, R.COEF_SETS["dense"])
    for t in (0, 1):
        p, ctype = R.container(9, -12345, R.COEF_SETS["dense"], init, inter, t)
        assert ctype == t and p[:3] == bytes([9, 0x40 | t, 8]) and np.array_equal(R.decode(nr, nc, p), want)
    assert R.m32_seq(init) == oracle.m32_encode_seq(init)


def test_chunk_bits_add_up_to_the_text():
    """the chunks' code bits are the segment's text: the bit store's growth less the serialised tree"""
    v = make_tile("sparse_big", 40, 60)
    _, _, init, inter = R.predict(40, 60, v)
    for stream in (init, inter):
        m = R.m32_seq(stream)
        _, end, cl, tree_bits = oracle.huffman_encode(m)
        bits = R.chunk_bits(stream, cl)
        assert len(bits) == -(-len(stream) // R.CHUNK) and sum(bits) == end - tree_bits
        assert bits[0] == sum(int(cl[b]) for x in stream[:R.CHUNK] for b in oracle.m32_encode(x))
    assert R.segment_code_lengths([3, 3, 3])[1] == 1 and R.segment_code_lengths(init)[1] > 1


# ---- the tiles of tests/lsop08_cases.py have the properties the GPU tests need
@pytest.mark.parametrize("shape", [(4, 4), (66, 66)], ids=lambda s: "%dx%d" % s)
def test_threshold_tiles_lie_either_side_of_two_to_the_53(shape):
    nr, nc = shape
    n_int = R.n_interior(nr, nc)
    m = K.largest_exact_magnitude(n_int)
    assert m * m * n_int < 2 ** 53 <= (m + 1) ** 2 * n_int
    tiles = K.threshold_tiles(nr, nc)
    assert sorted(tiles) == sorted(["at-mid", "at-row0", "at-last", "over-mid", "over-row0", "over-last", "int32min"])
    for name, v in tiles.items():
        assert (K.bound(nr, nc, v) < 2 ** 53) == name.startswith("at-"), name
        assert R.predict(nr, nc, v) is not None, name
        # on the exact side every sum of the normal equations is an integer the scan-order FP64 sums hold exactly
        if name.startswith("at-") and n_int <= 16:
            s, c = R.gram(nr, nc, v)
            es, ec = R.gram_exact(nr, nc, v)
            assert [int(x) for x in s] == es and all(int(c[a][b]) == ec[a][b] for a in range(9) for b in range(a, 9))
    for where in ("mid", "row0", "last"):
        a, b = tiles["at-" + where].astype(np.int64), tiles["over-" + where].astype(np.int64)
        assert (a != b).sum() == 1 and (b - a).max() == 1 and a.max() == m and b.max() == m + 1
    assert tiles["at-row0"][:nc].max() == m and tiles["at-last"][-1] == m and int(tiles["int32min"].min()) == R.I32_MIN


def test_single_symbol_tiles():
    nr, nc, v = K.single_symbol_first()
    seed, u, init, inter = R.predict(nr, nc, v)
    assert set(init) == {0} and K.distinct_bytes(init) == 1 and K.distinct_bytes(inter) > 1
    assert oracle.huffman_encode(R.m32_seq(init))[1] == 17            # the whole first segment: 17 tree bits, no text
    found = K.single_symbol_second()
    assert found is not None, "no all-equal interior within %d seeds a shape" % K.SECOND_SEARCH_SEEDS
    nr, nc, v, seed_no = found
    print("all-equal interior: %d x %d, seed %d" % (nr, nc, seed_no))
    _, _, init, inter = R.predict(nr, nc, v)
    assert K.distinct_bytes(inter) == 1 and K.distinct_bytes(init) > 1
    b0, end0, _, _ = oracle.huffman_encode(R.m32_seq(init))
    assert oracle.huffman_encode(R.m32_seq(inter), end0, b0)[1] == end0 + 17        # ... and the second one behind a first with text
    for name, p, want in K.single_symbol_containers():
        assert np.array_equal(R.decode(6, 7, p), want), name
    # the forms' sizes: 17 tree bits and no text for a segment of one symbol
    both = [p for name, p, _ in K.single_symbol_containers() if name == "both"][0]
    assert len(both) == R.HEADER_BYTES + (17 + 17 + 7) // 8


@pytest.mark.parametrize("shape", K.MAX_BODY_SHAPES, ids=lambda s: "%dx%d" % s)
def test_max_packing_holds_the_longest_bodies(shape):
    """gf_lsop08_max_packing "always fits": 32-bit noise makes every residual five or six M32 bytes, and the tiles with the most
    distinct bytes make the serialised trees as large as the shape allows; either container type"""
    import gridfour_amd
    nr, nc = shape
    cap = gridfour_amd.lib().gf_lsop08_max_packing(nr, nc)
    for name, v in K.max_body_tiles(nr, nc).items():
        seed, u, init, inter = R.predict(nr, nc, v)
        assert np.median([len(oracle.m32_encode(x)) for x in init + inter]) >= 5, name
        if name == "bytes" and shape in ((33, 65), (6, 257)):
            assert K.distinct_bytes(inter) == 256 and (K.distinct_bytes(init) == 256 or shape == (33, 65))
        for t in (0, 1):
            assert len(R.container(0, seed, u, init, inter, t)[0]) <= cap, (name, t)


def test_window_overflow_tile():
    """the tile of the packer's direct route: one chunk of the interior stream beyond the 2,048-word window by the margin of
    lsop08_cases.OVERFLOW_MARGIN_BITS, another inside it, no code longer than 56 bits (about 6 s: tiles of more than a million cells)"""
    o = K.overflow_tile()
    print("side %d, %d noise row(s), largest chunk %d bits, smallest %d, chunks beyond the window %d of %d, longest codes %r, tried %r" %
          (o.side, o.rows, max(o.chunk_bits), min(o.chunk_bits), sum(b > K.WINDOW_BITS for b in o.chunk_bits), len(o.chunk_bits), o.max_code,
           o.tried))
    assert o.side * o.side <= K.OVERFLOW_MAX_CELLS and o.tried[0][:2] == (1024, 4)
    assert max(o.chunk_bits) > K.WINDOW_BITS + K.OVERFLOW_MARGIN_BITS and min(o.chunk_bits) < K.WINDOW_BITS - 31
    assert max(o.max_code) <= K.MAX_CODE_BITS
    assert o.pack[:3] == bytes([6, 0x40, 8]) and len(o.pack) > R.HEADER_BYTES + sum(o.chunk_bits) // 8


def _sample14(golden_dir):
    (packing,) = tile_packings(os.path.join(golden_dir, "ref_samples", "Sample14_LSOP.gvrs"))[0]
    return oracle.lsop12_decode(101, 101, packing)


def test_lu_against_exact_rational_solve(golden_dir):
    """The float32 coefficients of the restated JAMA LU equal those of the exact solution of the integer system (0 ulp)."""
    cases = [("sample14", 101, 101, _sample14(golden_dir)), ("smooth", 33, 65, make_tile("smooth", 33, 65)),
             ("terrain0", 33, 65, R.terrain(33, 65, 0)), ("noise16", 33, 65, make_tile("noise16", 33, 65)),
             ("noise8", 16, 16, make_tile("noise8", 16, 16)), ("noise32", 16, 16, make_tile("noise32", 16, 16)),
             ("noise8", 7, 9, make_tile("noise8", 7, 9))]
    for name, nr, nc, v in cases:
        u, exact = R.coefficients(nr, nc, v), R.coefficients_exact(nr, nc, v)
        assert u is not None and exact is not None, name
        assert u.tobytes() == exact.tobytes(), (name, u, exact)


def test_wrong_rounding_changes_residuals():
    """floor(p + 0.5), LSOP12's rounding, is not (int)(p + 0.5f): the two differ on negative predictions."""
    for v, nr, nc in ((make_tile("smooth", 16, 16), 16, 16), (R.terrain(33, 65, 0), 33, 65)):
        u = R.coefficients(nr, nc, v)
        good, bad = R.interior(nr, nc, v, u), R.interior(nr, nc, v, u, rounding=R.estimate_floor)
        n_diff = sum(a != b for a, b in zip(good, bad))
        assert n_diff > len(good) // 10, n_diff
        assert not np.array_equal(R.reconstruct(nr, nc, int(v[0]), R.initialisers(nr, nc, v), good, u, rounding=R.estimate_floor), v)
    assert (R.estimate(-2.5), R.estimate_floor(-2.5)) == (-2, -2) and (R.estimate(-2.75), R.estimate_floor(-2.75)) == (-2, -3)
    assert R.estimate(float("nan")) == 0 and R.estimate(1e30) == 2 ** 31 - 1 and R.estimate(-1e30) == -2 ** 31
    assert R.estimate(np.float32(8388609.0)) == 8388610        # p + 0.5f is a float32 addition: it rounds to even at 2^23


def test_damaged_containers_are_refused():
    v = R.terrain(7, 9, 0)
    for t in (0, 1):
        p = R.encode(1, 7, 9, v, force_type=t)[0]
        with pytest.raises(IOError):
            R.decode(7, 9, p[:2] + bytes([12]) + p[3:])
        with pytest.raises(IOError):
            R.decode(7, 9, p[:1] + bytes([0x42]) + p[2:])
        with pytest.raises(IOError):
            R.decode(7, 9, p[:39] + struct.pack("<i", 10 ** 6) + p[43:])
        with pytest.raises(IOError):
            R.decode(7, 9, p[:50])


# ---- the library without a device ----
def test_size_functions():
    import gridfour_amd
    L = gridfour_amd.lib()
    for nr, nc in BOTH_TYPES + DEFLATE_ONLY + [(120, 150)]:
        n = L.gf_lsop08_residual_count(nr, nc)
        assert n == R.n_init(nr, nc) + R.n_interior(nr, nc)
        cap = L.gf_lsop08_max_packing(nr, nc)
        assert cap % 16 == 0 and cap >= 47 + 2 * 321 + 6 * n and cap >= 47 + 6 * n + 256
    for nr, nc in ((3, 9), (9, 3), (0, 5), (-1, -1)):
        assert L.gf_lsop08_residual_count(nr, nc) == 0 and L.gf_lsop08_max_packing(nr, nc) == 0
    # the restatement's packings fit
    for nr, nc, v in ((7, 9, make_tile("noise32", 7, 9)), (33, 65, make_tile("noise32", 33, 65))):
        for t in (0, 1):
            assert len(R.encode(0, nr, nc, v, force_type=t)[0]) <= L.gf_lsop08_max_packing(nr, nc)


def test_argument_refusals_without_a_device():
    import gridfour_amd
    from gridfour_amd import _lib
    L = gridfour_amd.lib()
    buf = np.zeros(64, np.int32)
    p = C.c_void_p(buf.ctypes.data)
    n = C.c_size_t(0)
    assert L.gf_lsop08_predict_dev(None, 7, 9, 1, p, p, 128, p, p) == _lib.ERR_ARG
    assert L.gf_lsop08_reconstruct_dev(None, 7, 9, 1, p, 128, p, None, p, p) == _lib.ERR_ARG
    assert L.gf_lsop08_encode_batch_i32_dev(None, 0, 7, 9, 1, p, p, 1024, p, p, p, 128, p, p) == _lib.ERR_ARG
    assert L.gf_lsop08_decode_batch_i32_dev(None, 7, 9, 1, p, 64, None, 64, p, p, p, p, 128, p, p) == _lib.ERR_ARG
    assert L.gf_lsop08_encode_batch_i32(None, 0, 7, 9, 1, p, p, 256, p, None, p) == _lib.ERR_ARG
    assert L.gf_lsop08_decode_batch_i32(None, 7, 9, 1, p, p, p, p) == _lib.ERR_ARG
    assert L.gf_lsop08_encode_i32(None, 0, 7, 9, p, p, 256, C.byref(n)) == _lib.ERR_ARG
    assert L.gf_lsop08_decode_i32(None, 7, 9, p, 64, p) == _lib.ERR_ARG


def test_python_binding_has_the_methods_of_the_lsop12_one():
    import gridfour_amd
    for name in ("encode", "encodeFloats", "implementsFloatingPointEncoding", "implementsIntegerEncoding", "decode", "decodeFloats",
                 "encode_batch", "decode_batch", "predict", "reconstruct"):
        assert callable(getattr(gridfour_amd.LsCodecHip, name)) and callable(getattr(gridfour_amd.LsCodec08Hip, name)), name


def test_java_adapter_and_shim_kind():
    """org.gridfour.hip.LsCodec08Hip implements both plug-in interfaces through the existing native encode / decode with a kind of
    its own, and the shim maps that kind to the gf_lsop08_* calls (no JDK in the image: checked as text)."""
    java = open(os.path.join(ROOT, "gridfour_amd", "java", "org", "gridfour", "hip", "LsCodec08Hip.java")).read()
    assert re.search(r"class\s+LsCodec08Hip\s+implements\s+ICompressionEncoder\s*,\s*ICompressionDecoder", java)
    assert re.search(r"public\s+LsCodec08Hip\s*\(\s*\)", java)
    assert "native" not in re.sub(r"/\*.*?\*/|//[^\n]*", "", java.replace("HipCodecNative", ""), flags=re.S)
    m = re.search(r"HipCodecNative\.KIND_LSOP08", java)
    assert m and "HipCodecNative.encode(" in java and "HipCodecNative.decode(" in java
    native = open(os.path.join(ROOT, "gridfour_amd", "java", "org", "gridfour", "hip", "HipCodecNative.java")).read()
    kind = re.search(r"KIND_LSOP08\s*=\s*(\d+)\s*;", native)
    assert kind
    shim = open(os.path.join(ROOT, "gridfour_amd", "java", "gvrs_hip_jni.cpp")).read()
    assert "gf_lsop08_encode_i32" in shim and "gf_lsop08_decode_i32" in shim and "gf_lsop08_max_packing" in shim
    assert re.search(r"KIND_LSOP08\s*=\s*%s\b" % kind.group(1), shim)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert 'addCompressionCodec("LSOP08", LsCodec08Hip.class, LsCodec08Hip.class)' in integ.replace("org.gridfour.hip.", "")
