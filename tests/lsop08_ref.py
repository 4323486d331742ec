"""An independent statement of the LSOP08 codec (lsop/LsOptimalPredictor08.java:56-160, 181-246, lsop/LsEncoder08.java:66-137,
lsop/LsDecoder08.java:71-163, lsop/LsHeader.java:137-189, 210-265, util/jama/LUDecomposition.java:70-134, 253-284): the yardstick of
the gf_lsop08_* entry points.  No reference-made LSOP08 file exists, so parity rests on reading the source and on the checks of
tests/test_lsop08_ref.py.

float32 arithmetic is done with numpy float32 scalars, FP64 with Python floats, the JAMA loops are written out.  The sums and the
interior stream also have numpy array forms (gram_fast, interior_fast) that give the same bits, which tests/test_lsop08_ref.py
checks; predict() and encode() use them, so that a tile of a million cells takes seconds.  The oracle supplies
only what the reference fixtures already pin: CodecM32 (m32_encode_seq / m32_decode_seq) and the legacy Huffman coder
(huffman_encode / huffman_decode with bit_pos / prefix).  Deflate is Python's zlib at level 6.
"""
import math
import struct
import zlib
from fractions import Fraction

import numpy as np

import oracle

F32 = np.float32
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
N_COEF = 8
HEADER_BYTES = 47                 # codec index, type | 0x40, 8, seed, 8 floats, the two M32 byte counts
COEF_OFFSET_REVISED, COEF_OFFSET_LEGACY = 7, 6
TYPE_HUFFMAN, TYPE_DEFLATE = 0, 1


def _wrap(x):
    return (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31


def n_init(nr, nc):
    return 2 * nc + 2 * nr - 5


def n_interior(nr, nc):
    return (nr - 2) * (nc - 2)


def java_int_cast(x):
    """(int) of a float: truncation toward zero, NaN -> 0, saturating (JLS 5.1.3)."""
    x = F32(x)
    if math.isnan(x):
        return 0
    if math.isinf(x):
        return I32_MAX if x > 0 else I32_MIN
    return max(I32_MIN, min(I32_MAX, math.trunc(Fraction(float(x)))))


def estimate(p):
    """(int)(p + 0.5f): a float32 addition, then Java's cast (LsOptimalPredictor08.java:147)."""
    with np.errstate(all="ignore"):
        return java_int_cast(F32(F32(p) + F32(0.5)))


def estimate_floor(p):
    """A WRONG rounding, floor(p + 0.5) as LSOP12's StrictMath.round does it, which the tests must tell apart from estimate()."""
    p = F32(p)
    if math.isnan(p):
        return 0
    if math.isinf(p):
        return I32_MAX if p > 0 else I32_MIN
    return max(I32_MIN, min(I32_MAX, math.floor(Fraction(float(p)) + Fraction(1, 2))))


def neighbours(idx, nc):
    """The neighbours of cell idx in the order of the eight coefficients (LsOptimalPredictor08.java:139-146)."""
    return (idx - 1, idx - nc - 1, idx - nc, idx - 2, idx - nc - 2, idx - 2 * nc - 2, idx - 2 * nc - 1, idx - 2 * nc)


def predict_f32(u, v, idx, nc):
    """u0 * z1 + ... + u7 * z8 in float32, left to right, one int -> float conversion per term."""
    nb = neighbours(idx, nc)
    p = None
    with np.errstate(all="ignore"):
        for i in range(8):
            t = F32(u[i]) * F32(v[nb[i]])
            p = t if p is None else F32(p + t)
    return p


# ---- the normal equations and JAMA's LU ----
def gram(nr, nc, v):
    """s[9], c[9][9] (upper triangle) accumulated in FP64 in scan order, multiply and add rounded separately (:186-210)."""
    s = [0.0] * 9
    c = [[0.0] * 9 for _ in range(9)]
    for r in range(2, nr):
        for col in range(2, nc):
            i = r * nc + col
            z = [float(v[i])] + [float(v[k]) for k in neighbours(i, nc)]          # z0 = the cell, z1 .. z8 in coefficient order (:192-200)
            for a in range(9):
                s[a] += z[a]
            for a in range(9):
                za = z[a]
                ca = c[a]
                for b in range(a, 9):
                    ca[b] += za * z[b]
    return s, c


def gram_fast(nr, nc, v):
    """The same sums with numpy: elementwise float64 products (each rounded once) and np.cumsum, which adds one element after the
    other in scan order -- the bits of gram(), at a hundredth of the time (tests/test_lsop08_ref.py holds the two together)."""
    g = np.asarray(v, np.int32).reshape(nr, nc).astype(np.float64)
    offs = [(0, 0), (0, -1), (-1, -1), (-1, 0), (0, -2), (-1, -2), (-2, -2), (-2, -1), (-2, 0)]
    z = [g[2 + dr:nr + dr, 2 + dc:nc + dc].ravel() for dr, dc in offs]
    s = [float(np.cumsum(z[a])[-1]) for a in range(9)]
    c = [[0.0] * 9 for _ in range(9)]
    for a in range(9):
        for b in range(a, 9):
            c[a][b] = float(np.cumsum(z[a] * z[b])[-1])
    return s, c


def gram_exact(nr, nc, v):
    """The same sums as exact integers."""
    v = [int(x) for x in v]
    s = [0] * 9
    c = [[0] * 9 for _ in range(9)]
    for r in range(2, nr):
        for col in range(2, nc):
            i = r * nc + col
            z = [v[i]] + [v[k] for k in neighbours(i, nc)]
            for a in range(9):
                s[a] += z[a]
                for b in range(a, 9):
                    c[a][b] += z[a] * z[b]
    return s, c


def system(s, c):
    """The bordered 9 x 9 design matrix and its right-hand side (:211-235)."""
    zero = s[0] * 0
    full = [[c[min(i, j)][max(i, j)] for j in range(9)] for i in range(9)]
    m = [[zero] * 9 for _ in range(9)]
    for i in range(1, 9):
        for j in range(1, 9):
            m[i - 1][j - 1] = full[i][j]
        m[i - 1][8] = s[i]
    for j in range(1, 9):
        m[8][j - 1] = s[j]
    b = [full[0][i] for i in range(1, 9)] + [s[0]]
    return m, b


def jama_solve(m, b):
    """LUDecomposition(A).solve(b) in FP64 (LUDecomposition.java:70-134, 253-284); None where isNonsingular() fails."""
    n = 9
    lu = [[float(x) for x in row] for row in m]
    piv = list(range(n))
    for j in range(n):
        col = [lu[i][j] for i in range(n)]
        for i in range(n):
            row = lu[i]
            s = 0.0
            for k in range(min(i, j)):
                s += row[k] * col[k]
            col[i] -= s
            row[j] = col[i]
        p = j
        for i in range(j + 1, n):
            if abs(col[i]) > abs(col[p]):
                p = i
        if p != j:
            lu[p], lu[j] = lu[j], lu[p]
            piv[p], piv[j] = piv[j], piv[p]
        if lu[j][j] != 0.0:
            for i in range(j + 1, n):
                lu[i][j] /= lu[j][j]
    if any(lu[j][j] == 0.0 for j in range(n)):
        return None
    x = [float(b[piv[i]]) for i in range(n)]
    for k in range(n):
        for i in range(k + 1, n):
            x[i] -= x[k] * lu[i][k]
    for k in range(n - 1, -1, -1):
        x[k] /= lu[k][k]
        for i in range(k):
            x[i] -= x[k] * lu[i][k]
    return x


def rational_solve(m, b):
    """The same system solved exactly (Gauss-Jordan over Fractions); None where it is singular."""
    n = 9
    a = [[Fraction(x) for x in row] + [Fraction(y)] for row, y in zip(m, b)]
    for j in range(n):
        p = next((i for i in range(j, n) if a[i][j] != 0), None)
        if p is None:
            return None
        a[j], a[p] = a[p], a[j]
        inv = 1 / a[j][j]
        a[j] = [x * inv for x in a[j]]
        for i in range(n):
            if i != j and a[i][j] != 0:
                f = a[i][j]
                a[i] = [x - f * y for x, y in zip(a[i], a[j])]
    return [a[i][n] for i in range(n)]


def coefficients(nr, nc, v, fast=True):
    """computeCoefficients, cast to float32; None where the reference returns null or JAMA throws."""
    if nr < 4 or nc < 4:
        return None
    s, c = (gram_fast if fast else gram)(nr, nc, v)
    x = jama_solve(*system(s, c))
    if x is None:
        return None
    with np.errstate(all="ignore"):
        return np.array([F32(x[i]) for i in range(8)], np.float32)


def coefficients_exact(nr, nc, v):
    """The exact rational solution of the integer system, rounded once to float32 (None: singular)."""
    x = rational_solve(*system(*gram_exact(nr, nc, v)))
    if x is None:
        return None
    return np.array([F32(float(x[i])) if abs(x[i]) < 2 ** 200 else F32(math.copysign(math.inf, x[i])) for i in range(8)], np.float32)


# ---- the two streams ----
def initialisers(nr, nc, v):
    """2 nC + 2 nR - 5 values (LsOptimalPredictor08.java:77-104), wrapping int32."""
    v = [int(x) for x in v]
    out = []
    for i in range(1, nc):
        out.append(_wrap(v[i] - v[i - 1]))
    prior = v[0]
    for i in range(nc):
        out.append(_wrap(v[nc + i] - prior))
        prior = v[nc + i]
    for r in range(2, nr):
        i = r * nc
        out.append(_wrap(v[i] - v[i - nc]))
        out.append(_wrap(v[i + 1] - v[i]))
    return out


def interior(nr, nc, v, u, rounding=estimate, trace=None):
    """(nR - 2)(nC - 2) residuals (:135-150); trace receives every prediction p."""
    v = [int(x) for x in v]
    uf = [F32(x) for x in np.asarray(u, np.float32)]
    out = []
    for r in range(2, nr):
        for c in range(2, nc):
            i = r * nc + c
            p = predict_f32(uf, v, i, nc)
            if trace is not None:
                trace.append(p)
            out.append(_wrap(v[i] - rounding(p)))
    return out


def interior_fast(nr, nc, v, u):
    """interior() with numpy float32 arrays: the int -> float32 conversion of every neighbour, the eight float32 products summed left
    to right (an elementwise numpy operation rounds once, as the scalar one does), + 0.5f, and Java's cast -- NaN -> 0, toward zero,
    saturating -- on the float64 image of the float32 sum, which is exact.  tests/test_lsop08_ref.py holds it to interior()."""
    g = np.asarray(v, np.int32).reshape(nr, nc)
    offs = [(0, -1), (-1, -1), (-1, 0), (0, -2), (-1, -2), (-2, -2), (-2, -1), (-2, 0)]          # neighbours(), as (row, column) steps
    uf = np.asarray(u, np.float32)
    with np.errstate(all="ignore"):
        p = None
        for i, (dr, dc) in enumerate(offs):
            t = uf[i] * g[2 + dr:nr + dr, 2 + dc:nc + dc].astype(np.float32)
            p = t if p is None else p + t
        assert p.dtype == np.float32
        q = (p + F32(0.5)).astype(np.float64)
        est = np.clip(np.trunc(np.where(np.isnan(q), 0.0, q)), float(I32_MIN), float(I32_MAX)).astype(np.int64)
    res = g[2:, 2:].astype(np.int64) - est
    return ((res + 2 ** 31) % 2 ** 32 - 2 ** 31).ravel().tolist()


def predict(nr, nc, v):
    """LsOptimalPredictor08.encode: (seed, u float32[8], initialisers, interior) or None (declined)."""
    u = coefficients(nr, nc, v)
    if u is None:
        return None
    return int(v[0]), u, initialisers(nr, nc, v), interior_fast(nr, nc, v, u)


def reconstruct(nr, nc, seed, init, inter, u, rounding=estimate, trace=None):
    """LsDecoder08.unpackInitializers + unpackInterior (:118-163)."""
    v = [0] * (nr * nc)
    init = [int(x) for x in init]
    inter = [int(x) for x in inter]
    k = 0
    v[0] = acc = int(seed)
    for i in range(1, nc):
        acc = _wrap(acc + init[k]); k += 1
        v[i] = acc
    acc = int(seed)
    for i in range(nc):
        acc = _wrap(acc + init[k]); k += 1
        v[nc + i] = acc
    for r in range(2, nr):
        o = r * nc
        v[o] = _wrap(v[o - nc] + init[k]); k += 1
        v[o + 1] = _wrap(v[o] + init[k]); k += 1
    uf = [F32(x) for x in np.asarray(u, np.float32)]
    ki = 0
    for r in range(2, nr):
        for c in range(2, nc):
            i = r * nc + c
            p = predict_f32(uf, v, i, nc)
            if trace is not None:
                trace.append(p)
            v[i] = _wrap(rounding(p) + inter[ki])
            ki += 1
    return np.array(v, np.int64).astype(np.int32)


# ---- the container ----
def pack_header(codec_index, ctype, seed, u, n_mi, n_mx):
    """LsHeader.packHeader with nCoefficients = 8, no checksum: 47 bytes."""
    return (struct.pack("<BBBi", codec_index & 0xFF, ctype | 0x40, N_COEF, _wrap(seed)) + np.asarray(u, "<f4").tobytes() +
            struct.pack("<ii", n_mi, n_mx))


def huffman_body(m_init, m_int):
    """HuffmanEncoder.encode of the initialiser bytes, then of the interior bytes, into one bit store."""
    b0, end0, _, _ = oracle.huffman_encode(m_init, 0, b"")
    b1, end1, _, _ = oracle.huffman_encode(m_int, end0, b0)
    return b1[:(end1 + 7) // 8]


class DeflateOverrun(Exception):
    """zlib needs more than n + 128 bytes for a stream: the reference would write a truncated packing (LsEncoder08.java:90-101);
    the library answers GF_ERR_UNSUPPORTED for such a tile."""


def deflate_body(m_init, m_int):
    z0, z1 = zlib.compress(m_init, 6), zlib.compress(m_int, 6)
    if len(z0) > len(m_init) + 128 or len(z1) > len(m_int) + 128:
        raise DeflateOverrun()
    return z0 + z1


def m32_seq(values):
    """oracle.m32_encode_seq, with the oracle asked once per distinct value (a stream of a million values has a few thousand)."""
    vals = [int(x) for x in values]
    code = {x: oracle.m32_encode(x) for x in set(vals)}
    return b"".join([code[x] for x in vals])


def container(codec_index, seed, u, init, inter, ctype=None):
    """LsEncoder08.encode :85-134 from the two streams on: (packing, type).  ctype None: the reference's choice, Huffman only where
    its body is strictly shorter; 0 / 1: that container whatever its size (the device encoder writes type 0 always)."""
    m_init, m_int = m32_seq(init), m32_seq(inter)
    body_h = huffman_body(m_init, m_int)
    if ctype is None:
        body_d = deflate_body(m_init, m_int)
        ctype = TYPE_DEFLATE if len(body_h) >= len(body_d) else TYPE_HUFFMAN
    body = body_h if ctype == TYPE_HUFFMAN else deflate_body(m_init, m_int)
    return pack_header(codec_index, ctype, seed, u, len(m_init), len(m_int)) + body, ctype


def encode(codec_index, nr, nc, v, force_type=None):
    """LsEncoder08.encode: (packing, type) or (None, None).  force_type: see container()."""
    pr = predict(nr, nc, v)
    if pr is None:
        return None, None
    return container(codec_index, *pr, ctype=force_type)


CHUNK = 1024                      # values of a chunk of k_lsop8_pack (L8_THREADS * P8_VPT)


def segment_code_lengths(stream):
    """(code_lengths[256] of HuffmanEncoder for the stream's M32 bytes, number of distinct bytes); the single-symbol form has no
    text: every length is 0"""
    m = np.frombuffer(m32_seq(stream), np.uint8)
    return oracle.huffman_encode(m)[2].astype(np.int64), int(np.unique(m).size)


def chunk_bits(stream, code_lengths):
    """code bits of each run of CHUNK consecutive values of a stream: for every value the code lengths of its M32 bytes, summed"""
    vals = np.asarray([int(x) for x in stream], np.int64)
    uniq, inv = np.unique(vals, return_inverse=True)
    cl = np.asarray(code_lengths, np.int64)
    per = np.array([int(cl[np.frombuffer(oracle.m32_encode(int(x)), np.uint8)].sum()) for x in uniq], np.int64)[inv]
    return [int(per[i:i + CHUNK].sum()) for i in range(0, len(per), CHUNK)]


def parse_header(pack):
    """LsHeader(packing, 0): either revision, a value checksum skipped.  Returns (type, seed, u, nMI, nMX, header size)."""
    if len(pack) < 3:
        raise IOError("short header")
    o = 1
    revised = bool(pack[1] & 0x40)
    ctype = checksum = None
    if revised:
        ctype, checksum = pack[1] & 0x0F, bool(pack[1] & 0x80)
        o = 2
    if len(pack) < o + 1 + 4 + 4 * N_COEF + 8 + (0 if revised else 1):
        raise IOError("short header")
    if pack[o] != N_COEF:
        raise IOError("not an 8-coefficient container")
    o += 1
    seed, = struct.unpack_from("<i", pack, o)
    u = np.frombuffer(pack[o + 4:o + 4 + 4 * N_COEF], "<f4").copy()
    o += 4 + 4 * N_COEF
    n_mi, n_mx = struct.unpack_from("<ii", pack, o)
    o += 8
    if not revised:
        ctype, checksum = pack[o] & 0x0F, bool(pack[o] & 0x80)
        o += 1
    if checksum:
        o += 4
    if o > len(pack):
        raise IOError("short header")
    return ctype, seed, u, n_mi, n_mx, o


def decode(nr, nc, pack):
    """LsDecoder08.decode; IOError where the container cannot be read (the library's negative statuses)."""
    pack = bytes(pack)
    ctype, seed, u, n_mi, n_mx, o = parse_header(pack)
    if ctype not in (TYPE_HUFFMAN, TYPE_DEFLATE):
        raise IOError("container type %d" % ctype)
    ni, nx = n_init(nr, nc), n_interior(nr, nc)
    if n_mi < 0 or n_mx < 0 or n_mi > 6 * ni + 64 or n_mx > 6 * nx + 64:
        raise IOError("counts no encoder emits")
    body = pack[o:]
    try:
        if ctype == TYPE_HUFFMAN:
            m_init, pos = oracle.huffman_decode(body, n_mi, 0)
            if pos > 8 * len(body):
                raise IOError("initialiser segment ends early")
            m_int, pos = oracle.huffman_decode(body, n_mx, pos)
            if pos > 8 * len(body):
                raise IOError("interior segment ends early")
        else:
            d = zlib.decompressobj()
            m_init = d.decompress(body)
            if not d.eof or len(m_init) < n_mi:
                raise IOError("initialiser stream")
            d2 = zlib.decompressobj()
            m_int = d2.decompress(d.unused_data)
            if not d2.eof or len(m_int) < n_mx:
                raise IOError("interior stream")
            m_init, m_int = m_init[:n_mi], m_int[:n_mx]
    except (ValueError, zlib.error) as e:
        raise IOError(str(e))
    init, used0 = oracle.m32_decode_seq(m_init, ni)
    inter, used1 = oracle.m32_decode_seq(m_int, nx)
    if used0 > len(m_init) or used1 > len(m_int):
        raise IOError("M32 bytes end early")
    return reconstruct(nr, nc, seed, init, inter, u)


def substitute(pack, u, legacy=False):
    """The container with its eight coefficients replaced."""
    o = COEF_OFFSET_LEGACY if legacy else COEF_OFFSET_REVISED
    b = bytearray(pack)
    b[o:o + 32] = np.asarray(u, "<f4").tobytes()
    return bytes(b)


def to_legacy_header(pack):
    """A revised-header packing rearranged into the legacy header (LsHeader.java:140-160): the type byte moves behind the counts."""
    assert pack[1] & 0x40
    return bytes(pack[:1]) + bytes(pack[2:HEADER_BYTES]) + bytes([pack[1] & 0x8F]) + bytes(pack[HEADER_BYTES:])


def with_checksum_flag(pack, value=0x12345678):
    """A revised-header packing with bit 7 set and four checksum bytes behind the counts (the decoders skip them)."""
    assert pack[1] & 0x40
    return bytes(pack[:1]) + bytes([pack[1] | 0x80]) + bytes(pack[2:HEADER_BYTES]) + struct.pack("<I", value) + bytes(pack[HEADER_BYTES:])


# ---- tiles and coefficient sets shared by the tests ----
def terrain(nr, nc, seed=0, amp=800):
    """The _terrain generator of tests/test_gpu_lsop.py."""
    rng = np.random.default_rng(seed * 7919 + nr * 131 + nc)
    y, x = np.mgrid[0:nr, 0:nc]
    return (amp * np.sin(x / 9.0) * np.cos(y / 7.0) + 50 * np.sin(x * y / 300.0) + rng.integers(-3, 4, (nr, nc))).astype(np.int32).ravel()


def _u(*pairs):
    u = np.zeros(8, np.float32)
    for i, x in pairs:
        u[i] = x
    return u


NAN, INF = float("nan"), float("inf")
COEF_SETS = {
    # half of the left neighbour: p is x.5 or an integer; p + 0.5f lands on an integer for every odd neighbour, of both signs
    "half_left": _u((0, 0.5)),
    "neg_half_left": _u((0, -0.5)),             # negative predictions: truncation and floor differ by one
    "minus_up": _u((2, -1.0)),                  # p = -(cell above): negative integers, p + 0.5 truncates back to p
    "quarters": _u((0, 0.25), (2, 0.75)),
    "average": _u((0, 0.5), (2, 0.5)),
    "dense": np.array([0.31, -0.17, 0.23, 0.11, -0.07, 0.19, 0.13, 0.27], np.float32),
    "sat_pos": _u((0, 1e30)),                   # saturation at both int32 limits
    "sat_neg": _u((0, -1e30)),
    "pos_inf": _u((0, INF)),                    # +-Inf, and Inf - Inf = NaN -> estimate 0
    "neg_inf": _u((2, -INF)),
    "inf_pair": _u((0, INF), (3, -INF)),
    "nan": _u((4, NAN), (0, 1.0)),
    "neg_zero": np.full(8, -0.0, np.float32),
}
