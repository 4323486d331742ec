"""An independent statement of LsDecoder12's reconstruction (lsop/LsDecoder12.java:186-221, 311-383) and the tiles and coefficient
sets that the LSOP12 numeric tests share.

The prediction is the float32 sum of LsOptimalPredictor12.java:254-267, multiplied and added left to right with numpy float32
scalars; StrictMath.round(float) is restated with exact rationals: floor(p + 1/2), NaN -> 0, saturating at the int32 limits.  Test
containers are made by COEFFICIENT SUBSTITUTION: an oracle-made container with its twelve stored floats overwritten.  The residual
streams do not change, so a decoder routes the tile exactly as before while its predictions become whatever the coefficients make them.
"""
import math
from fractions import Fraction

import numpy as np

import oracle

F32 = np.float32
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1

# where the twelve coefficients lie in a container: LsHeader.packHeader (LsHeader.java:210-264) writes codec, type byte, 12, seed,
# then the floats; the legacy header (LsHeader.java:139-160) has no type byte in front of the 12
COEF_OFFSET_REVISED, COEF_OFFSET_LEGACY = 7, 6


def java_round_float(p):
    """StrictMath.round(float): floor(p + 1/2) exactly, NaN -> 0, saturating."""
    p = F32(p)
    if math.isnan(p):
        return 0
    if math.isinf(p):
        return I32_MAX if p > 0 else I32_MIN
    f = math.floor(Fraction(float(p)) + Fraction(1, 2))
    return max(I32_MIN, min(I32_MAX, f))


def round_half_even(p):
    """A WRONG rounding (ties to even) that the tie sets below must tell apart from java_round_float."""
    p = F32(p)
    if math.isnan(p):
        return 0
    if math.isinf(p):
        return I32_MAX if p > 0 else I32_MIN
    return max(I32_MIN, min(I32_MAX, round(Fraction(float(p)))))


# the neighbours of cell idx in the order of the twelve coefficients (LsOptimalPredictor12.java:254-267)
def neighbours(idx, nc):
    return (idx - 1, idx - nc - 1, idx - nc, idx - nc + 1, idx - nc + 2, idx - 2, idx - nc - 2,
            idx - 2 * nc - 2, idx - 2 * nc - 1, idx - 2 * nc, idx - 2 * nc + 1, idx - 2 * nc + 2)


def predict_f32(u, v, idx, nc, order=range(12)):
    """u[0] * z1 + ... + u[11] * z12 in float32, left to right (order: a permutation, for the tests that show order matters)."""
    nb = neighbours(idx, nc)
    p = None
    with np.errstate(all="ignore"):
        for i in order:
            t = F32(u[i]) * F32(v[nb[i]])
            p = t if p is None else F32(p + t)
    return p


def _wrap(x):
    return (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31


def reconstruct(nr, nc, seed, init, interior, u, rounding=java_round_float, order=range(12), trace=None):
    """LsDecoder12.unpackInitializers + unpackInterior: residual streams and coefficients -> the tile (int32 wrap-around).
    trace (a list, optional) receives every interior prediction p."""
    v = [0] * (nr * nc)
    init = [int(x) for x in init]
    interior = [int(x) for x in interior]
    k = 0
    v[0] = int(seed)
    acc = int(seed)
    for i in range(1, nc):
        acc = _wrap(acc + init[k]); k += 1
        v[i] = acc
    acc = int(seed)
    for i in range(1, nr):
        acc = _wrap(acc + init[k]); k += 1
        v[i * nc] = acc

    def tri(idx):
        nonlocal k
        v[idx] = _wrap(init[k] + (v[idx - 1] + v[idx - nc]) - v[idx - nc - 1])
        k += 1

    for i in range(1, nc):
        tri(nc + i)
    for i in range(2, nr):
        tri(i * nc + 1)
    ki = 0
    uf = [F32(x) for x in np.asarray(u, np.float32)]
    for r in range(2, nr):
        for c in range(2, nc - 2):
            idx = r * nc + c
            p = predict_f32(uf, v, idx, nc, order)
            if trace is not None:
                trace.append(p)
            v[idx] = _wrap(rounding(p) + interior[ki])
            ki += 1
        tri(r * nc + nc - 2)
        tri(r * nc + nc - 1)
    return np.array(v, np.int64).astype(np.int32)


def substitute(pack, u, legacy=False):
    """The container with its twelve coefficients replaced (value checksum off: the cells change)."""
    o = COEF_OFFSET_LEGACY if legacy else COEF_OFFSET_REVISED
    b = bytearray(pack)
    b[o:o + 48] = np.asarray(u, "<f4").tobytes()
    return bytes(b)


def stored_coefficients(pack, legacy=False):
    o = COEF_OFFSET_LEGACY if legacy else COEF_OFFSET_REVISED
    return np.frombuffer(pack[o:o + 48], "<f4").copy()


def container_type(pack):
    return pack[1] & 0x0F if pack[1] & 0x40 else None


def plane_geom_ok(nr, nc):
    """gf_lsop_plane_geom(nR, nC).ok (gvrs_kernels.h:292-309), restated: the shapes whose byte-residual tiles decode as a plane."""
    if nr < 6 or nc < 32 or nc > 4096 or nr > 1024:
        return False
    n_init, n_int, lanes = 4 * nr + 2 * nc - 9, (nr - 2) * (nc - 4), 32
    p = (max(nc, 112) + 15) & ~15
    n_ph = (nr - 2 + lanes - 1) // lanes
    n_last = nr - 2 - lanes * (n_ph - 1)
    s_end = (n_ph - 1) * p + 3 * (n_last - 1) + nc - 1
    n_blocks = s_end // 16 + 1
    off_words = (n_init + 3) & ~3
    rows_words = 2 * (96 + p + 32)
    lds_bytes = (2 * rows_words + 64 * 33 + 128) * 4
    return off_words * 4 + n_blocks * lanes * 16 <= (n_init + n_int) * 4 and lds_bytes <= 64 * 1024


def byte_residuals(nr, nc, v):
    """True when every interior residual of the tile lies in -127..127 (k_lsop_unpack2 then writes a byte plane)."""
    ref = oracle.lsop12_residuals(nr, nc, v)
    return ref is not None and int(np.abs(ref[3].astype(np.int64)).max()) <= 127


# ---- tiles ----
def smooth(nr, nc, seed=0, offset=0, amp=400):
    """Terrain whose LSOP12 interior residuals are bytes (the kind of tile the plane kernel takes)."""
    rng = np.random.default_rng(seed + 17 * nr + nc)
    y, x = np.mgrid[0:nr, 0:nc]
    v = amp * np.sin(x / 17.0 + seed) * np.cos(y / 13.0) + 150 * np.sin((x + 2 * y) / 29.0) + rng.integers(-2, 3, (nr, nc))
    return (v.astype(np.int64) + offset).astype(np.int32).ravel()


def with_spike(v, nr, nc, r, c, delta):
    """One interior cell moved by delta: one interior residual wider than a byte, so the tile keeps the int32 residual array."""
    v = v.copy()
    v[r * nc + c] += delta
    return v


# ---- coefficient sets; each says what it makes the predictions do ----
def _u(*pairs):
    u = np.zeros(12, np.float32)
    for i, x in pairs:
        u[i] = x
    return u


NAN, INF = float("nan"), float("inf")
COEF_SETS = {
    # half of the left neighbour: exact .5 predictions of both signs wherever it is odd (-2.5 must round to -2, 2.5 to 3)
    "tie_pos": _u((0, 0.5)),
    "tie_neg": _u((0, -0.5)),
    # quarters and three-quarters: fractions .25, .5, .75; a sum of one, so the values stay near the tile's own
    "quarters": _u((0, 0.25), (2, 0.75)),
    "three_quarters": _u((0, 0.75), (1, -0.25), (2, 0.5)),
    # the average of the left and upper neighbours: on a tile near 2^22 (float32 spacing 0.5) p is an exact x.5 in [2^22, 2^23);
    # near 2^24 and beyond the neighbours themselves round when converted to float
    "average": _u((0, 0.5), (2, 0.5)),
    # a realistic predictor with inexact weights (sum 1): near 2^21 the partial sums round at every step, so the order of the twelve
    # additions decides the last bit, and with a spacing of 0.25 that decides the rounding often
    "inexact": np.array([0.1, 0.2, 0.3, 0.4, -0.1, -0.2, 0.15, 0.05, -0.05, 0.1, 0.02, 0.03], np.float32),
    "dense": np.array([0.31, -0.17, 0.23, 0.11, -0.07, 0.19, 0.13, -0.29, 0.37, -0.03, 0.21, 0.01], np.float32),
    # large terms that cancel with small ones between them (left - two-left at 1e8): reordering the additions changes the result
    "cancel": np.array([1e8, 0.3, 0.7, -0.2, 0.1, -1e8, 0.05, 0.4, -0.3, 0.2, 0.1, -0.05], np.float32),
    # saturation at both ends: p far beyond +-2^31 (the value is the saturated estimate + residual, wrapped), then +-inf and NaN
    "sat_pos": _u((0, 1e30)),
    "sat_neg": _u((0, -1e30)),
    "sat_both": _u((0, 1e30), (2, -1e30)),
    # non-finite coefficients: +-inf times a neighbour is +-inf (saturated estimates of both signs); inf - inf is NaN (estimate 0), after
    # which cells equal their residuals, often 0, and inf * 0 is NaN as well
    "pos_inf": _u((0, INF)),
    "neg_inf": _u((2, -INF)),
    "inf_pair": _u((0, INF), (5, -INF)),
    "nan": _u((3, NAN), (0, 1.0)),
    # zeros and subnormals: estimate 0 everywhere, -0.0 sums, products that underflow to (signed) zero
    "neg_zero": np.full(12, -0.0, np.float32),
    "subnormal": _u((0, 1e-45), (1, -1e-40), (2, 1.0), (9, 1e-39)),
}


# (coefficient set, value offset of the source tile): the offsets put the predictions where float32 spacing is 0.5 (6,000,000 ~ 2^22.5),
# 0.25 (3,000,000) and 2 (20,000,000 > 2^24)
CASES = [(name, 0) for name in COEF_SETS] + [("average", 6_000_000), ("average", 20_000_000), ("inexact", 3_000_000),
                                             ("inexact", 6_000_000), ("dense", 3_000_000), ("tie_pos", 6_000_000),
                                             ("quarters", 3_000_000)]
# the cases whose decoded tiles change when any two of the twelve additions trade places (together; tests/test_oracle_lsop_numeric.py)
ORDER_CASES = [("inexact", 6_000_000), ("dense", 3_000_000)]


def case_id(case):
    return "%s@%d" % case if case[1] else case[0]


def tile_for(nr, nc, offset, seed=1):
    return smooth(nr, nc, seed, offset)
