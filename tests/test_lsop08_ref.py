"""CPU-only: the Python restatement of LSOP08 (tests/lsop08_ref.py) holds together -- it round-trips, its LU agrees with an exact
rational solve, its rounding is told apart from LSOP12's -- and what of the gf_lsop08_* family can be checked without a device: the
size functions, the argument refusals, the Java adapter and its shim kind (as text)."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest

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
