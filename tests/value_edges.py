"""Residual streams with chosen values at the edges of the integer codecs' encoding classes, and the tiles that carry them.

Two classifications decide the bytes of a residual:
  CodecM32 (CodecHuffman, CodecDeflate, LSOP12 legacy/Deflate containers; CodecM32.java encode :105-111 / decode): one byte for
    -126..126 and the null code (0x80), then 2..6 bytes -- introducer 0x7f / 0x81 and |v| - base in 7-bit groups -- with the
    bases 127, 255, 16,639, 2,113,791, 270,549,247.
  CanonicalHuffman (CodecCanonHuffman, LSOP12 current container; countSymbols :352-418, encode :203-276): kind 0 is -128..127,
    kinds 1-3 add one to three 2-bit escapes (+-512, +-2,048, +-8,192), kinds 4-6 one to three byte escapes (+-32,768,
    +-8,388,608, the rest), kind 7 is Integer.MIN_VALUE as the null symbol.  The emit side (:258) tests -8,333,608 where
    countSymbols (:395) tests -8,388,608: the values -8,388,608..-8,333,609 are counted as kind 5 and written as kind 6.

A tile is built from its residual stream: oracle.predictor_decode_int(model, seed, ...) of a background of small residuals with
the chosen values put at chosen stream positions; oracle.predictor_encode_int gives the same stream back
(tests/test_value_edges_oracle.py proves it for every tile made here).  The stream orders are the encoders' (gvrs_decode.hip,
"Stream layouts"): Differencing -- cell (r, c) at r nC + c - 1; Linear -- (0,1) at 0, (r,0) / (r,1) at 2r - 1 / 2r, the interior
of row r from 2 nR - 1 + r (nC - 2); Triangle -- row 0, then column 0, then the interior of row r >= 1 at nC + nR - 2 +
(r - 1)(nC - 1); DifferencingWithNulls -- every cell in row order, (0,0) included."""
import struct
import zlib

import numpy as np

import oracle

NULL = -2 ** 31
IMAX = 2 ** 31 - 1
DIFF, LINEAR, TRIANGLE, NULLS = 1, 2, 3, 4           # GF_PM_* / the predictor byte of a packing

# ---- the two classifications restated

M32_BASES = (127, 255, 16639, 2113791, 270549247)    # first |v| of 2..6 bytes (CodecM32.java :105-111)


def m32_len(v):
    """bytes of v in CodecM32 (the null code is the one byte 0x80)"""
    v = int(v)
    if v == NULL:
        return 1
    a = abs(v)
    return 1 if a <= 126 else 1 + sum(a >= b for b in M32_BASES)


GAP = (-8388608, -8333609)                           # counted as kind 5 (:395), written as kind 6 (:258)
CANON_KIND_RANGES = ((0, -128, 127), (1, -512, 511), (2, -2048, 2047), (3, -8192, 8191), (4, -32768, 32767),
                     (5, -8388608, 8388607))


def canon_kind(v):
    """countSymbols :352-418: 0 plain, 1..3 that many 2-bit escapes, 4..6 that many byte escapes, 7 the null symbol"""
    v = int(v)
    if v == NULL:
        return 7
    for k, lo, hi in CANON_KIND_RANGES:
        if lo <= v <= hi:
            return k
    return 6


def canon_emit_kind(v):
    """the kind CanonicalHuffman.encode :203-276 writes: as countSymbols but for the lower bound of kind 5 (:258)"""
    v = int(v)
    k = canon_kind(v)
    return 6 if k == 5 and v < -8333608 else k


def canon_target(v):
    """the standard symbol of the first code countSymbols counts for v (CN_NULL for the null code)"""
    k = canon_kind(v)
    if k == 7:
        return 256
    return (int(v) >> (0, 2, 4, 6, 8, 16, 24)[k]) + 128


def in_gap(v):
    return GAP[0] <= int(v) <= GAP[1]


# ---- the edge sets of the issue table

def _pm(xs):
    return [s * x for x in xs for s in (1, -1)]


# both ends of every M32 length with both signs; -127 / -128: two-byte values with payload 0x00 / 0x01
M32_EDGES = tuple(sorted(set(_pm([126, 127, 128, 254, 255, 16638, 16639, 2113790, 2113791, 270549246, 270549247, IMAX])
                             + [NULL, 0, 1, -1])))
# the lowest and highest value of each canonical kind and one past each (the ends give target symbols 0 and 255), both ends of the
# gap and the first value written as kind 5 after it, the top of the int range and the null symbol
CANON_EDGES = tuple(sorted(set([-128, 127, -129, 128, -512, 511, -513, 512, -2048, 2047, -2049, 2048, -8192, 8191, -8193, 8192,
                                -32768, 32767, -32769, 32768, -8388608, 8388607, -8388609, 8388608, GAP[0], GAP[1], GAP[1] + 1,
                                IMAX, -IMAX, NULL])))
WIDE = tuple(v for v in M32_EDGES if m32_len(v) >= 2)
WIDE56 = tuple(v for v in M32_EDGES if m32_len(v) >= 5)
NARROW_WIDE = tuple(v for v in M32_EDGES if 2 <= m32_len(v) <= 3)


# ---- stream positions

def n_residuals(model, nr, nc):
    return nr * nc if model == NULLS else nr * nc - 1


def stream_index(model, nr, nc, r, c):
    """position of cell (r, c)'s residual in the model's stream"""
    if model in (DIFF,):
        return r * nc + c - 1
    if model == NULLS:
        return r * nc + c
    if model == LINEAR:
        if r == 0 and c == 1:
            return 0
        if c < 2:
            return 2 * r - 1 + c
        return 2 * nr - 1 + r * (nc - 2) + (c - 2)
    if model == TRIANGLE:
        if r == 0:
            return c - 1
        if c == 0:
            return nc - 2 + r
        return nc + nr - 2 + (r - 1) * (nc - 1) + (c - 1)
    raise ValueError(model)


def placements(model, nr, nc):
    """{name: stream position} of the cells each predictor treats differently"""
    last = n_residuals(model, nr, nc) - 1
    at = lambda r, c: stream_index(model, nr, nc, r, c)
    if model == DIFF:
        p = {"first(0,1)": at(0, 1), "col0(1,0)": at(1, 0), "col0(r,0)": at(nr // 2, 0), "lastcol(r,nc-1)": at(nr // 2, nc - 1),
             "interior": at(nr // 2, nc // 2)}
    elif model == LINEAR:
        p = {"first(0,1)": at(0, 1), "(r,0)": at(nr // 2, 0), "(r,1)": at(nr // 2, 1), "(0,2)": at(0, 2),
             "interior": at(nr // 2, nc // 2)}
    elif model == TRIANGLE:
        p = {"first(0,1)": at(0, 1), "row0": at(0, nc // 2), "col0": at(nr // 2, 0), "(1,1)": at(1, 1),
             "interior": at(nr // 2, nc // 2)}
    else:
        raise ValueError(model)
    p["last"] = last
    return p


# ---- tiles from residual streams

def background(model, nr, nc, seed, lo=-3, hi=3):
    rng = np.random.default_rng(seed * 7919 + model * 131 + nr * 17 + nc)
    return rng.integers(lo, hi + 1, n_residuals(model, nr, nc)).astype(np.int64)


def tile_from_residuals(model, nr, nc, residuals, seed=1000):
    """the tile whose model-stream is exactly residuals (models 1-3: no cell may come out as the null code)"""
    res = (np.asarray(residuals, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    v = oracle.predictor_decode_int(model, seed, nr, nc, res)
    return v, res


def edge_tile(model, nr, nc, placed, seed=1000, bg_seed=0, bg=None):
    """tile with placed = [(position, residual), ...] over a background of small residuals.  Where a cell of a model 1-3 tile
    would come out as the null code (a wide residual on the wrong value), the background is drawn again."""
    for k in range(64):
        res = (background(model, nr, nc, bg_seed + 1000 * k) if bg is None else np.array(bg, np.int64))
        for pos, val in placed:
            res[pos] = val
        v, r32 = tile_from_residuals(model, nr, nc, res, seed)
        if model == NULLS or not (v == NULL).any():
            return v, r32
        if bg is not None:
            break
    raise AssertionError("no background keeps the null code out of the tile (model %d, %dx%d)" % (model, nr, nc))


def value_tiles(model, nr, nc, values, seed=1000, bg_seed=0):
    """one tile per value: the value at every placement of the model (one distinct wide value in an otherwise one-byte tile)"""
    pos = sorted(set(placements(model, nr, nc).values()))
    out = []
    for i, e in enumerate(values):
        out.append(edge_tile(model, nr, nc, [(p, e) for p in pos], seed + i, bg_seed + i))
    return out


def gap_tiles(model, nr, nc, seed=1500):
    """the two ends of the gap over a background with and without the value -1: encode writes a gap value as symbol 127 (the
    value -1, (v >> 24) + 128) and three byte escapes, where countSymbols counted symbol 0 (:258 vs :395); the packing reads back
    only where -1 has a code of its own.  Returns [(tile, residuals, background has -1)]"""
    out = []
    for k, (lo, hi) in enumerate(((-3, 3), (0, 3))):
        for e in GAP:
            bg = background(model, nr, nc, seed + k, lo, hi)
            v, r = edge_tile(model, nr, nc, [(p, e) for p in sorted(set(placements(model, nr, nc).values()))], seed, bg=bg)
            out.append((v, r, lo < 0))
    return out


def phase_tiles(model, nr, nc, widths=(2, 3, 4, 5, 6), seed=2000):
    """one wide value per tile behind one-byte values, starting at each of the four byte phases of a dword; a six-byte value as
    the first residual and one as the last (the stream ends with its last byte); returns [(tile, residuals, position)]"""
    by_len = {n: [v for v in M32_EDGES if m32_len(v) == n] for n in widths}
    n = n_residuals(model, nr, nc)
    base = (n // 2) & ~3
    out = []
    for w in widths:
        for ph in range(4):
            e = by_len[w][ph % len(by_len[w])]
            v, r = edge_tile(model, nr, nc, [(base + ph, e)], seed + 10 * w + ph, w * 4 + ph)
            out.append((v, r, base + ph))
    for pos in (0, n - 1):
        for e in (IMAX, -IMAX):
            v, r = edge_tile(model, nr, nc, [(pos, e)], seed + pos + (e > 0), 77 + (e > 0))
            out.append((v, r, pos))
    return out


def dense_tile(model, nr, nc, values, frac, seed=3000, bg_seed=0):
    """values spread over a fraction frac of the stream positions (the first and the last position always among them)"""
    rng = np.random.default_rng(seed + nr * 3 + nc)
    n = n_residuals(model, nr, nc)
    pos = np.nonzero(rng.random(n) < frac)[0].tolist()
    pos = sorted(set(pos) | {0, n - 1})
    vals = np.asarray(values, np.int64)[rng.integers(0, len(values), len(pos))]
    return edge_tile(model, nr, nc, list(zip(pos, vals.tolist())), seed, bg_seed)


def m32_bytes(model, residuals):
    return len(oracle.m32_encode_seq(residuals))


def roomy_edge_tiles(model, nr, nc, n, plan, seed=4000):
    """tiles whose M32 stream lies between the fast run's budget and the roomy run's (plan: route_plan.plan of the batch), made of
    two- and three-byte edge values at a density found on the oracle's packing"""
    for q in (0.3, 0.2, 0.12, 0.06):
        tiles = [dense_tile(model, nr, nc, NARROW_WIDE, q, seed + t, t) for t in range(n)]
        nm = [m32_bytes(model, r) for _, r in tiles]
        if all(plan.fastM32 < x <= plan.ldsM32Roomy - 4096 for x in nm):
            return tiles
    raise AssertionError("no density of edge values puts a %dx%d tile between the fast and the roomy budget" % (nr, nc))


def general_edge_tile(model, nr, nc, seed=5000):
    """five- and six-byte edge values at most positions: the stream outgrows every LDS budget (more than 4 bytes per cell)"""
    return dense_tile(model, nr, nc, WIDE56, 0.8, seed, 1)


def rare_edge_tile(nr, nc, seed=6000, n_wide=3):
    """Differencing residuals with a geometric spread (codes of 15 bits and more) and a few five- and six-byte edge values:
    their bytes are rare, so M32 bytes per value x the longest code passes 64 bits (k_huffman_pack_rare)"""
    rng = np.random.default_rng(seed + nr + nc)
    n = nr * nc - 1
    res = (rng.geometric(0.5, n) - 1) * rng.choice((-1, 1), n)
    pos = rng.choice(np.arange(1, n - 1), n_wide, replace=False).tolist() + [n - 1]
    vals = [WIDE56[(seed + i) % len(WIDE56)] for i in range(len(pos) - 1)] + [IMAX]
    return edge_tile(DIFF, nr, nc, list(zip(pos, vals)), 1000, bg=res)


def int_min_tiles(nr, nc, seed=7000):
    """Integer.MIN_VALUE as a genuine residual of models 1-3 (M32 byte 0x80, the canonical null symbol): it must decode as a value"""
    out = []
    for model in (DIFF, LINEAR, TRIANGLE):
        pos = sorted(set(placements(model, nr, nc).values()))
        out.append((model,) + edge_tile(model, nr, nc, [(p, NULL) for p in pos], seed + model, model))
    return out


def _run_starts(null, nc):
    """cells where a run of DifferencingWithNulls starts over at the seed: (0,0), a cell after a null inside a row, a row start
    whose row above starts with a null (the encoder's nullFlag, PredictorModelDifferencingWithNulls.java:169-237)"""
    n = null.size
    return [0] + [i for i in range(1, n) if not null[i] and (null[i - nc] if i % nc == 0 else null[i - 1])]


def nulls_tile(nr, nc, values, seed=1000, bg_seed=0):
    """DifferencingWithNulls: null runs, the chosen values right after each run start and right before each null, each followed by
    its negation where the run goes on (so the run returns near the seed and no cell of the tile is the null code by accident).
    Run-start residuals are 0: every run starts at the seed, and the encoder's seed -- the rounded mean of the run starts -- is
    the seed again.  (Sums that land on the null code cannot come from a tile: see nulls_sum_stream.)"""
    rng = np.random.default_rng(bg_seed * 31 + nr + nc)
    n = nr * nc
    res = rng.integers(-3, 4, n).astype(np.int64)
    null = np.zeros(n, bool)
    for _ in range(max(2, n // 40)):
        a = int(rng.integers(1, n - 3))
        null[a:a + int(rng.integers(1, 6))] = True
    null[nc:nc + 3] = True                                   # a run at the start of row 1
    null[-1] = False
    res[null] = NULL
    starts = _run_starts(null, nc)
    res[starts] = 0
    taken = set(starts)

    def free(i):
        return 0 <= i < n and not null[i] and i % nc != 0 and i not in taken

    vals = [v for v in values if v != NULL]
    j = 0
    for i in [s + 1 for s in starts] + [i - 1 for i in range(1, n) if null[i] and not null[i - 1]]:
        if free(i):
            res[i] = vals[j % len(vals)]
            taken.add(i)
            if free(i + 1):
                res[i + 1] = -res[i]
                taken.add(i + 1)
            j += 1
    return tile_from_residuals(NULLS, nr, nc, res, seed)


def _wrap32(x):
    return (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31


def nulls_sum_stream(nr, nc, values, seed=5, rng_seed=0):
    """A hand-made DifferencingWithNulls residual stream (no encoder writes one) in which sums land on the null code next to edge
    values: in every row an edge value, then the residual that takes the sum to Integer.MIN_VALUE, then an edge value again (the
    row goes on from that sum); every other row starts with a sum of MIN_VALUE too (the next row then starts from the seed,
    PredictorModelDifferencingWithNulls.decode :137-166, test_gpu_deflate.py).  The residuals that aim at MIN_VALUE are worked
    out on the oracle's decode of the stream so far.  Returns (seed, residuals, {cells decoded as MIN_VALUE from a sum})."""
    assert nc >= 5
    rng = np.random.default_rng(rng_seed * 101 + nr * 7 + nc)
    n = nr * nc
    res = rng.integers(-3, 4, n).astype(np.int64)
    res[rng.random(n) < 0.1] = NULL
    vals = [v for v in values if v != NULL]

    def decoded():
        return oracle.predictor_decode_int(NULLS, seed, nr, nc, (res & 0xFFFFFFFF).astype(np.uint32).view(np.int32))

    def aim(i):                                            # residual at i that makes cell i MIN_VALUE (prior: cell i - 1's sum)
        res[i] = 0
        res[i] = _wrap32(NULL - int(decoded()[i]))

    sums = set()
    for r in range(nr):
        o = r * nc
        if r % 2 == 1:
            aim(o)
            sums.add(o)
        c = 1 + int(rng.integers(0, nc - 4))
        res[o + c] = vals[(2 * r) % len(vals)]
        aim(o + c + 1)
        res[o + c + 2] = vals[(2 * r + 1) % len(vals)]
        sums.add(o + c + 1)
    return seed, (res & 0xFFFFFFFF).astype(np.uint32).view(np.int32), sums


def nulls_sum_packings(nr, nc, seed, residuals):
    """CodecDeflate (zlib), CodecHuffman and raw (header + M32 bytes) containers of predictor 4 around a residual stream"""
    m32 = oracle.m32_encode_seq(np.asarray(residuals, np.int64).astype(np.int32))
    head = bytes([0, NULLS]) + struct.pack("<iI", seed, len(m32))
    return (head + zlib.compress(m32, 6), oracle.huffman_encode(np.frombuffer(m32, np.uint8), 80, head)[0], head + m32)


# ---- saturated one-byte tiles for the byte path

def saturated_tile(model, nr, nc, value, seed=1000):
    """every residual of the model's stream equal to value (+126: the top of the byte path's biased 16-bit column sums, -126:
    the bottom); the cells wrap as int32 sums do and none may be the null code"""
    res = np.full(n_residuals(model, nr, nc), value, np.int64)
    for s in range(seed, seed + 64):
        v, r = tile_from_residuals(model, nr, nc, res, s)
        if not (v == NULL).any():
            return v, r
    raise AssertionError("every seed puts the null code into a saturated tile")


def byte_path_scratch_words(threads):
    """SCR_WORDS of the k_huffman_decode build (gvrs_decode.hip: offsetof(DecShared, waveSum) / 4): lut 4 KB, leafCode 2 KB,
    leafLen / leafSym / shortLeaf 576 B, qs / qe / qn / qdirty 13 B per subsequence (MAXQ = 512 for the 256- and the 512-thread
    build, 1,024 for the 1024-thread one, build.py), head 88 words.
    A restatement of the DecShared layout: the library exposes no such number.  What pins it on the device is
    test_gpu_value_edges.test_byte_path_saturated_tiles: on the 512- and the 1024-thread build the shapes byte_path_limit_shapes
    picks sit at the fused stage's ring limit (fused_ring, the same words), and the retry word must say the general kernel got
    the tile one row taller and not the tile itself -- a layout change moves the limit and fails that test."""
    maxq = 512 if threads <= 512 else 1024
    return (4096 + 2048 + 576 + 13 * maxq + 4 * 88) // 4


def byte_path_eligible(model, nr, nc, lds_m32, threads):
    """gvrs_decode.hip byte_path_eligible, restated"""
    waves = threads // 64
    rb = (nr + waves - 1) // waves
    scr = byte_path_scratch_words(threads)
    return (1 <= model <= 3 and nr >= 2 and nc >= 4 and nc <= 256 and rb <= 255 and nr * nc + 8 <= lds_m32
            and ((2 * nr + 3) & ~3) + (waves * ((nc + 3) & ~3) if model == 3 else 0) <= scr)


def fused_ring(model, nr, nc, threads):
    """gvrs_decode.hip fused_plan(...).ring != 0 for models 1-3: without a ring the fast kernel leaves the tile to the general one
    (GF_K_RETRY) before the byte path is considered; two row arrays (three for Linear), nC and FUSED_CHUNK = 4 x threads words"""
    rows = (3 if model == LINEAR else 2) * nr
    return nr >= 2 and nc >= 4 and nc <= 2 * threads and nr <= 4096 and rows + nc + 4 * threads + 1 <= byte_path_scratch_words(threads)


def byte_path_limit_shapes():
    """(build, nR, nC) per k_huffman_decode build and residue of nC mod 4: the first column count from 4 on (up to 256, the byte
    path's limit) for which the build's byte path takes a Differencing tile whose next row count it does not take, at the tallest
    such row count (route_plan.plan picks the build, byte_path_eligible and fused_ring decide).  The 256-thread build stops at
    RB = 255 rows per wave; the 512- and the 1024-thread builds stop earlier, where the fused stage's ring runs out of words."""
    import route_plan as rp
    out = []
    for threads in rp.BUILDS:
        waves = threads // 64
        found = {}
        for nc in range(4, 257):
            if nc % 4 in found:
                continue
            top = min(255 * waves, (byte_path_scratch_words(threads) - nc - 4 * threads - 1) // 2)
            for nr in range(top, max(1, top - 64), -1):
                p = rp.plan(rp.KIND_HUFFMAN, nr, nc, 4)
                if p.decThreads == threads and byte_path_eligible(DIFF, nr, nc, p.fastM32, threads) and fused_ring(DIFF, nr, nc, threads):
                    q = rp.plan(rp.KIND_HUFFMAN, nr + 1, nc, 4)
                    if not (byte_path_eligible(DIFF, nr + 1, nc, q.fastM32, q.decThreads) and fused_ring(DIFF, nr + 1, nc, q.decThreads)):
                        found[nc % 4] = (threads, nr, nc)
                    break
            if len(found) == 4:
                break
        out += [found[k] for k in sorted(found)]
    return out


# ---- hand-made LSOP12 containers around chosen residual streams

def lsop_n_init(nr, nc):
    return 4 * nr + 2 * nc - 9


def lsop_n_interior(nr, nc):
    return (nr - 2) * (nc - 4)


def _lsop_head(codec_index, typ, seed, coefs, checksum, counts):
    """LsHeader.packHeader :210-265 (the revised form): codec, type | 0x40 | checksum flag, 12, seed, 12 floats, the two code
    counts (types 0 and 1 only), the checksum"""
    h = bytes([codec_index, typ | 0x40 | (0x80 if checksum else 0), 12]) + struct.pack("<i", seed)
    h += np.asarray(coefs, "<f4").tobytes()
    if counts is not None:
        h += struct.pack("<ii", *counts)
    if checksum:
        h += b"\x12\x34\x56\x78"
    return h


def lsop_deflate_container(seed, coefs, init, interior, checksum=False, codec_index=0):
    """a type-1 container (LsEncoder12.encode :170-205): the two M32 streams, each its own zlib stream at level 6"""
    m_init, m_int = oracle.m32_encode_seq(init), oracle.m32_encode_seq(interior)
    head = _lsop_head(codec_index, 1, seed, coefs, checksum, (len(m_init), len(m_int)))
    return head + zlib.compress(m_init, 6) + zlib.compress(m_int, 6)


def lsop_canon_container(seed, coefs, init, interior, checksum=False, codec_index=0):
    """a type-2 container (LsEncoder12.encode :140-160, gvrs_oracle_lsop.c): the initialisers and the interior as two canonical
    Huffman texts in one bit store behind the header"""
    head = _lsop_head(codec_index, 2, seed, coefs, checksum, None)
    buf, pos, _ = oracle.canon_encode(np.asarray(init, np.int64).astype(np.int32), len(head) * 8, head)
    buf, pos, _ = oracle.canon_encode(np.asarray(interior, np.int64).astype(np.int32), pos, buf)
    return buf


def lsop_streams(nr, nc, values, seed=0):
    """(initialisers, interior) of the LSOP12 stream lengths: small background, values at the first and the last position of each
    stream and spread through both"""
    rng = np.random.default_rng(seed * 13 + nr + nc)
    ni, nx = lsop_n_init(nr, nc), lsop_n_interior(nr, nc)
    init = rng.integers(-3, 4, ni).astype(np.int64)
    inter = rng.integers(-3, 4, nx).astype(np.int64)
    vals = list(values)
    for arr in (init, inter):
        k = len(arr)
        pos = sorted(set([0, k - 1] + rng.choice(np.arange(1, k - 1), min(len(vals), k - 2), replace=False).tolist()))
        for j, p in enumerate(pos):
            arr[p] = vals[(j + seed) % len(vals)]
    return init, inter
