"""The LSOP12 prediction and its rounding at their numeric edges, CPU only: the oracle's decoder (java_round_float and lsop_predict,
oracle/gvrs_oracle_lsop.c:21-28, 108-140) against an independent Python statement of LsDecoder12's interior step (tests/lsop_ref.py:
numpy float32 left to right, StrictMath.round by exact rationals).  The containers are oracle-made with their coefficients
substituted, so the residual streams stay as the encoder wrote them while the predictions hit ties, huge magnitudes, saturation,
infinities, NaN, zeros and subnormals.  The GPU kernels are then held to the oracle in tests/test_gpu_lsop_numeric.py."""

import numpy as np
import pytest

import lsop_ref as L
import oracle
from lsop_ref import CASES, COEF_SETS, F32, case_id

SHAPES = [(12, 16), (24, 40)]


def _source(nr, nc, offset, legacy=False):
    v = L.tile_for(nr, nc, offset)
    seed, _, init, interior = oracle.lsop12_residuals(nr, nc, v)
    if legacy:
        pack = oracle.lsop12_encode_legacy_huffman(3, nr, nc, v)
    else:
        pack, typ = oracle.lsop12_encode(3, nr, nc, v, False)
        assert typ == 2
    return pack, seed, init, interior


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_oracle_decode_equals_the_float32_statement(shape, case):
    nr, nc = shape
    name, offset = case
    u = COEF_SETS[name]
    pack, seed, init, interior = _source(nr, nc, offset)
    sub = L.substitute(pack, u)
    assert L.stored_coefficients(sub).tobytes() == u.tobytes()
    want = L.reconstruct(nr, nc, seed, init, interior, u)
    got = oracle.lsop12_decode(nr, nc, sub)
    assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:8])


@pytest.mark.parametrize("case", [("tie_neg", 0), ("sat_both", 0), ("inexact", 3_000_000)], ids=case_id)
def test_legacy_header_substitution(case):
    """The legacy header (coefficients at bytes 6..53) decodes to the same statement."""
    nr, nc = 24, 40
    name, offset = case
    pack, seed, init, interior = _source(nr, nc, offset, legacy=True)
    sub = L.substitute(pack, COEF_SETS[name], legacy=True)
    want = L.reconstruct(nr, nc, seed, init, interior, COEF_SETS[name])
    assert np.array_equal(oracle.lsop12_decode(nr, nc, sub), want)


def test_the_own_coefficients_give_the_tile_back():
    # (the statement is a decoder: with the encoder's coefficients it reproduces the tile, at every magnitude used here)
    for offset in (0, 3_000_000, 6_000_000, 20_000_000):
        v = L.tile_for(24, 40, offset)
        seed, u, init, interior = oracle.lsop12_residuals(24, 40, v)
        assert np.array_equal(L.reconstruct(24, 40, seed, init, interior, u), v), offset


def test_java_round_float_edges():
    r = L.java_round_float
    assert [r(F32(x)) for x in (2.5, -2.5, 0.5, -0.5, -1.5, 1.49999988, -0.49999997)] == [3, -2, 1, 0, -1, 1, 0]
    assert r(F32(4194304.5)) == 4194305 and r(F32(-4194304.5)) == -4194304          # 2^22 + 1/2: spacing 0.5
    assert r(F32(2.0 ** 31)) == L.I32_MAX and r(F32(-(2.0 ** 31))) == L.I32_MIN and r(F32(-(2.0 ** 31) - 256)) == L.I32_MIN
    assert r(F32(2147483520.0)) == 2147483520                                         # the largest float below 2^31
    assert r(F32("inf")) == L.I32_MAX and r(F32("-inf")) == L.I32_MIN and r(F32("nan")) == 0
    assert r(F32(1e-45)) == 0 and r(F32(-1e-45)) == 0 and r(F32(-0.0)) == 0
    assert L.round_half_even(F32(2.5)) == 2 and L.round_half_even(F32(-2.5)) == -2


def _trace(nr, nc, name, offset):
    pack, seed, init, interior = _source(nr, nc, offset)
    ps = []
    L.reconstruct(nr, nc, seed, init, interior, COEF_SETS[name], trace=ps)
    return np.array(ps, np.float32)


def test_the_sets_reach_what_they_target():
    """Each set makes the predictions do what its comment says, on the 24 x 40 source tile."""
    nr, nc = 24, 40
    p = _trace(nr, nc, "tie_pos", 0)
    assert np.any((p > 0) & (p - np.floor(p) == 0.5)) and np.any((p < 0) & (p - np.floor(p) == 0.5))
    p = _trace(nr, nc, "tie_neg", 0)
    assert np.any(p == -2.5) or np.any((p < 0) & (p - np.floor(p) == 0.5))
    p = _trace(nr, nc, "quarters", 0)
    assert {0.25, 0.5, 0.75} <= set((p - np.floor(p)).tolist())
    p = _trace(nr, nc, "average", 6_000_000)
    big = (np.abs(p) >= 2 ** 22) & (np.abs(p) < 2 ** 23)
    assert np.any(big & (p - np.floor(p) == 0.5))
    p = _trace(nr, nc, "average", 20_000_000)
    assert np.all(np.abs(p) >= 2 ** 24)
    for name in ("sat_pos", "sat_neg", "sat_both"):
        p = _trace(nr, nc, name, 0)
        assert np.any(np.abs(p.astype(np.float64)) >= 2.0 ** 31), name
    p = _trace(nr, nc, "sat_both", 0)
    assert np.any(p >= 2.0 ** 31) and np.any(p <= -(2.0 ** 31))
    for name in ("pos_inf", "neg_inf"):
        p = _trace(nr, nc, name, 0)
        assert np.any(np.isposinf(p)) and np.any(np.isneginf(p)), name
    for name in ("inf_pair", "nan"):
        assert np.any(np.isnan(_trace(nr, nc, name, 0))), name
    p = _trace(nr, nc, "neg_zero", 0)
    assert np.all(p == 0) and np.any(np.signbit(p))
    p = _trace(nr, nc, "subnormal", 0)
    assert np.all(np.isfinite(p))


@pytest.mark.parametrize("case", [("tie_pos", 0), ("tie_neg", 0), ("quarters", 0), ("average", 6_000_000), ("quarters", 3_000_000)],
                         ids=case_id)
def test_ties_to_even_would_be_caught(case):
    """Rounding ties to even instead of toward +infinity changes the decoded tile: the tie sets discriminate."""
    nr, nc = 24, 40
    name, offset = case
    pack, seed, init, interior = _source(nr, nc, offset)
    right = L.reconstruct(nr, nc, seed, init, interior, COEF_SETS[name])
    wrong = L.reconstruct(nr, nc, seed, init, interior, COEF_SETS[name], rounding=L.round_half_even)
    assert not np.array_equal(right, wrong)


def test_any_two_additions_swapped_would_be_caught():
    """Exchanging any two of the twelve terms of the float32 sum changes a decoded tile of ORDER_CASES (the first two terms excepted:
    t0 + t1 is t1 + t0).  "cancel" changes under some exchanges as well."""
    nr, nc = 24, 40
    srcs = []
    for name, offset in L.ORDER_CASES + [("cancel", 0)]:
        pack, seed, init, interior = _source(nr, nc, offset)
        srcs.append((name, seed, init, interior, L.reconstruct(nr, nc, seed, init, interior, COEF_SETS[name])))
    missed, cancel_caught = [], 0
    for i in range(12):
        for j in range(i + 1, 12):
            order = list(range(12))
            order[i], order[j] = order[j], order[i]
            changed = [not np.array_equal(right, L.reconstruct(nr, nc, seed, init, interior, COEF_SETS[name], order=order))
                       for name, seed, init, interior, right in srcs]
            if (i, j) != (0, 1) and not any(changed[:-1]):
                missed.append((i, j))
            cancel_caught += changed[-1]
    assert not missed, missed
    assert cancel_caught >= 30
