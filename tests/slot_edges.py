"""Families of small tiles whose packing lengths step through consecutive values, built with the oracle alone: what the encoder
write-bound tests (tests/test_gpu_encode_bounds.py) put around a slot stride S.

Construction: a smooth base tile, 300 sin(row / 5) cos(col / 4), with independent noise added to its first k cells, k = 0 .. cells:
the packing grows by about a byte per step, so that around a stride S (a multiple of 16, as the ABI asks) the lengths S - 3 .. S + 1
all occur -- a packing that just fits with its last 32-bit word filled in every way, and one that just does not.  Every family
picks its S from the oracle's lengths; tests/test_slot_edges_oracle.py holds, on the CPU, the conditions the GPU test relies on.

One family per packer path of the encoders (gvrs_encode.hip, gvrs_canon_encode.hip, gvrs_lsop.hip); where the path depends on the
tile's content, the property is proved on the oracle's residuals (is_plain, keeps_plane, rare_bits, lsop16_eligible below;
test_slot_edges_oracle.test_content_selects_the_packer), for the tiles that fit -- the others are never packed:
  huffman plane-m*      pack_plane_ranges<1..3>: a plain stream (every residual one M32 byte, no null), every row difference one byte
                        too (the phase-A kernel keeps the byte plane), nC >= CPT = 8
  huffman flatplain-m*  pack_flat_ranges<m, true>: plain, but nC = 4 < CPT
  huffman wide-m*       pack_flat_ranges<m, false> (pack_head for Linear and Triangle): a few residuals of two M32 bytes
  huffman nulls         model 4, pack_flat_ranges<4, false>
  huffman rare          k_huffman_pack_rare: M32 bytes per value x the longest code beyond the packer's window step
  huffman general       k_huffman_encode<false>: 6 cells >= 2^23
  canon plain-m*, nulls k_canon_pack without escapes;  canon escape: every escape kind 1..6 (value_edges.canon_kind)
  lsop 16 / 32          k_canon_pack2 with and without the 16-bit histogram records (gf_lsop_predict16_eligible, restated in
                        lsop16_eligible), each with and without GF_LSOP_VALUE_CHECKSUM (header 55 / 59 bytes)
  lsop08                k_lsop8_pack (gvrs_lsop8.hip; lengths from the restatement tests/lsop08_ref.py, type 0 as the device encoder
                        writes it): a shape whose cell count is no multiple of 4 and LSOP_WIDE
  m32                   k_m32_streams: three candidates per tile, written when length + 8 <= sub_stride
  canon uniform         the uniform form (6 bytes, predictor 0) at the smallest legal stride, 16: the only tiles that fit
(The canonical encoder also has an overflow branch for a uniform tile at strides below 8 (gvrs_canon_encode.hip, "early =
GF_K_OVERFLOW"): the ABI refuses a slot_stride below 16, so no call reaches it and nothing here tests it.)"""
import functools

import numpy as np

import lsop08_ref
import oracle
import value_edges as ve

NULL = ve.NULL
OK, DECLINED, OVERFLOW = 0, 1, 2
SENTINEL = 0xA5                      # what slots, guards and blobs hold before a call
GUARD = 4096                         # bytes before and behind a slot array (at least; see Family.guard)
NEAR = 20                            # lengths within S +- NEAR are taken one tile each
LSOP_CHECKSUM = 2                    # GF_LSOP_VALUE_CHECKSUM
LSOP_RING_MAXC = 256                 # gvrs_lsop.hip


def base_tile(nr, nc, amp=300.0):
    r, c = np.meshgrid(np.arange(nr), np.arange(nc), indexing="ij")
    return np.rint(amp * np.sin(r / 5.0) * np.cos(c / 4.0)).astype(np.int64).ravel()


def ladder(nr, nc, noise_amp=60, seed=5, spikes=(), null_block=None, cells_set=(), base=None):
    """k -> the base tile with the first k cells' noise added.  spikes: ((cell, height), ...) added to every tile of the ladder;
    null_block: (r0, r1, c0, c1) of null cells; cells_set: ((cell, value), ...) cells that hold a fixed value (no noise there)."""
    b = base_tile(nr, nc) if base is None else np.asarray(base, np.int64)
    noise = np.random.default_rng(seed).integers(-noise_amp, noise_amp + 1, nr * nc).astype(np.int64)
    for cell, _ in cells_set:
        noise[cell] = 0

    def tile(k):
        v = b.copy()
        v[:k] += noise[:k]
        for cell, h in spikes:
            v[cell:] += h                       # a step: one wide residual, the cells behind it stay smooth
        for cell, val in cells_set:
            v[cell] = val
        if null_block:
            r0, r1, c0, c1 = null_block
            m = v.reshape(nr, nc)
            m[r0:r1, c0:c1] = NULL
        return ((v + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)

    return tile


class Family:
    """tiles [n, cells] in batch order with the oracle's packing (None: declined), predictor and length of each, the stride S and
    the ladder's lengths (all_lengths: every length the construction reached, for the CPU conditions).
    m32 families: packs[t] = the three candidate streams (None: no candidate), lengths[t] = their lengths, preds[t] = their models."""

    def __init__(self, name, codec, nr, nc, mask=0xF, lsop_flags=0):
        self.name, self.codec, self.nr, self.nc, self.mask, self.lsop_flags = name, codec, nr, nc, mask, lsop_flags
        self.tiles, self.packs, self.preds, self.lengths = [], [], [], []
        self.seeds = []                       # m32 families: the seed of every tile (d_seeds)
        self.stride = 0
        self.all_lengths = []
        self.relaxed = False                  # huffman general: one packing within 16 bytes under S and one within 16 over

    @property
    def cells(self):
        return self.nr * self.nc

    @property
    def n(self):
        return len(self.tiles)

    def guard(self):
        """bytes before and behind the slot array: GUARD, and at least the longest packing of the family (whatever a wrong length
        or a packer that ignored the stride could write from the last slot's start stays inside the allocation)"""
        longest = max([max(x) if isinstance(x, tuple) else x for x in self.lengths] + [0])
        return max(GUARD, (longest + 15) // 16 * 16)

    def margin(self):
        """bytes a packing needs beyond its length (the M32 packer's whole-word flushes: 8)"""
        return 8 if self.codec == "m32" else 0

    def expected_status(self, t):
        if self.codec == "m32":
            return OVERFLOW if any(p is not None and len(p) + 8 > self.stride for p in self.packs[t]) else OK
        if self.packs[t] is None:
            return DECLINED
        return OVERFLOW if self.lengths[t] > self.stride else OK

    def values(self):
        return np.ascontiguousarray(np.stack(self.tiles), dtype=np.int32)


def encode_one(codec, nr, nc, tile, mask=0xF, lsop_flags=0):
    """(packing | None, predictor) by the oracle"""
    if codec == "huffman":
        return oracle.codec_huffman_encode(0, nr, nc, tile, predictor_mask=mask)
    if codec == "canon":
        return oracle.codec_canon_encode(0, nr, nc, tile, predictor_mask=mask)
    if codec == "lsop":
        pk, _ = oracle.lsop12_encode(0, nr, nc, tile, False, bool(lsop_flags & LSOP_CHECKSUM))
        return pk, 0
    if codec == "lsop08":
        return lsop08_ref.encode(0, nr, nc, tile, force_type=lsop08_ref.TYPE_HUFFMAN)[0], 0
    raise ValueError(codec)


def m32_candidates(nr, nc, tile):
    """the three sub-slots of gf_m32_encode_batch_i32_dev: (streams, models, seed); Differencing, Linear, Triangle, or the
    DifferencingWithNulls stream in sub-slot 0 of a tile with nulls (predictor_encode_int + m32_encode_seq)"""
    if (np.asarray(tile) == NULL).any():
        res, seed = oracle.predictor_encode_int(ve.NULLS, nr, nc, tile)
        return (oracle.m32_encode_seq(res), None, None), (ve.NULLS, 0, 0), seed
    out, seed = [], 0
    for model in (ve.DIFF, ve.LINEAR, ve.TRIANGLE):
        res, seed = oracle.predictor_encode_int(model, nr, nc, tile)
        out.append(oracle.m32_encode_seq(res))
    return tuple(out), (ve.DIFF, ve.LINEAR, ve.TRIANGLE), seed


def m32_stream_len(res):
    """bytes of a residual stream in CodecM32 (value_edges.m32_len over an array)"""
    a = np.abs(np.asarray(res, np.int64))
    n = 1 + sum((a >= b).astype(np.int64) for b in ve.M32_BASES)
    return int(np.where((a <= 126) | (np.asarray(res, np.int64) == NULL), 1, n).sum())


def m32_candidate_lengths(nr, nc, tile):
    """the lengths of m32_candidates' streams of a tile without nulls, without making the bytes"""
    return tuple(m32_stream_len(oracle.predictor_encode_int(m, nr, nc, tile)[0]) for m in (ve.DIFF, ve.LINEAR, ve.TRIANGLE))


def pick_stride(lengths, lo=16, offsets=(-3, -2, -1, 0, 1)):
    """the multiple of 16, from lo on, nearest the middle of the lengths for which S + o occurs for every o of offsets
    (S - 3 .. S: a last word filled in each of the four ways; S + 1: the first packing that does not fit); None where there is none"""
    have = set(lengths)
    mid = (min(have) + max(have)) // 2
    cands = [s for s in range(max(lo, 16), max(have) + 32, 16) if all(s + o in have for o in offsets)]
    return min(cands, key=lambda s: (abs(s - mid), s)) if cands else None


def _order(fit_edge, silent_over, rest, nulls, first, last):
    """batch order: `first` (a packing of exactly S bytes) leads; every tile with S - 3 <= L <= S is followed by a tile that writes
    nothing (an all-null tile or one with L > S, in turn); the other tiles; `last` (an edge tile again) ends the batch"""
    out = []
    over, k = list(silent_over), 0
    for e in [first] + [x for x in fit_edge if x is not first]:
        out.append(e)
        if k % 2 == 0 or not over:
            out.append(nulls)
        else:
            out.append(over.pop(0))
        k += 1
    for x in rest:
        out.append(x)
        if over:
            out.append(over.pop(0))
    out += over
    out.append(nulls)
    out.append(last)
    return out


def build_family(name, codec, nr, nc, tile_of, ks, mask=0xF, lsop_flags=0, lo=16, extra=()):
    """the family of a ladder: S from the lengths of tile_of(k), k in ks; one tile per length within S +- NEAR, three far below,
    three far above, `extra` tiles (far from S), all-null tiles in between"""
    f = Family(name, codec, nr, nc, mask, lsop_flags)
    enc = {}
    for k in ks:
        pk, pred = encode_one(codec, nr, nc, tile_of(k), mask, lsop_flags)
        assert pk is not None, (name, k)
        enc[k] = (pk, pred)
    lens = {k: len(enc[k][0]) for k in enc}
    f.all_lengths = sorted(set(lens.values()))
    S = pick_stride(lens.values(), lo)
    assert S is not None, "%s: no stride with S-3 .. S+1 among %d..%d" % (name, f.all_lengths[0], f.all_lengths[-1])
    f.stride = S
    by_len = {}
    for k in sorted(lens):
        by_len.setdefault(lens[k], k)                           # the first k of every length
    item = lambda k: (tile_of(k), enc[k][0], enc[k][1])
    near = [item(by_len[L]) for L in sorted(by_len) if abs(L - S) <= NEAR]
    far = sorted(L for L in by_len if abs(L - S) > NEAR)
    below = [item(by_len[L]) for L in far if L < S][:3]
    above = [item(by_len[L]) for L in far if L > S][-3:]
    for v in extra:
        pk, pred = encode_one(codec, nr, nc, v, mask, lsop_flags)
        assert pk is not None and abs(len(pk) - S) > NEAR
        (below if len(pk) < S else above).append((v, pk, pred))
    nulls = (np.full(nr * nc, NULL, np.int32), None, 0)
    fit_edge = sorted([x for x in near if S - 3 <= len(x[1]) <= S], key=lambda x: -len(x[1]))
    over = [x for x in near if len(x[1]) > S] + above
    rest = [x for x in near if len(x[1]) < S - 3] + below
    first = fit_edge[0]
    assert len(first[1]) == S
    last = next(x for x in fit_edge if len(x[1]) == S - 1)
    for v, pk, pred in _order(fit_edge, over, rest, nulls, first, last):
        f.tiles.append(v)
        f.packs.append(pk)
        f.preds.append(pred)
        f.lengths.append(len(pk) if pk is not None else 0)
    return f


# ---- content properties (proved on the oracle's residuals)

def residuals(model, nr, nc, tile):
    return oracle.predictor_encode_int(model, nr, nc, tile)[0].astype(np.int64)


def is_plain(model, nr, nc, tile):
    """every residual of the model's stream is one M32 byte and none is the null code (the packer's `plain`)"""
    res = residuals(model, nr, nc, tile)
    return bool((np.abs(res) <= 126).all())


def keeps_plane(nr, nc, tile):
    """no null cell and every row difference one byte (gvrs_encode.hip, phase A: "the byte plane holds this tile")"""
    v = np.asarray(tile, np.int64).reshape(nr, nc)
    return not (v == NULL).any() and bool((np.abs(np.diff(v, axis=1)) <= 126).all()) and bool((np.abs(np.diff(v[:, 0])) <= 126).all())


def rare_bits(nr, nc, tile, model):
    """M32 bytes of the widest value x the longest Huffman code of the packing's text (k_huffman_pack's `fast` test is
    STEP_CELLS x this <= (WIN_WORDS - 2) x 32; tests/test_gpu_value_edges._lean_pack_keeps)"""
    res = residuals(model, nr, nc, tile)
    max_len = int(oracle.huffman_encode(np.frombuffer(oracle.m32_encode_seq(res), np.uint8))[2].max())
    return max(ve.m32_len(x) for x in res) * max_len


def lsop16_eligible(nr, nc):
    """gf_lsop_predict16_eligible (gvrs_lsop.hip), restated: sizeof(LsopShared16) = 4,360 bytes (tests/test_gpu_lsop_numeric.py)"""
    cells, interior = nr * nc, (nr - 2) * (nc - 4)
    return nr >= 6 and nc >= 6 and nc <= LSOP_RING_MAXC and interior < (1 << 17) and 2 * ((cells + 64 + 15) & ~15) + 4360 <= 150 * 1024


# ---- the families

SMALL = (16, 40)
STRIP = (160, 4)
MASKS = {1: 1, 2: 2, 3: 4}                       # model -> predictor_mask
WIDE_SPIKES = ((97, 1000), (333, -1000), (571, 5000))
NULL_BLOCK = (5, 8, 10, 22)
LSOP_WIDE = (6, 257)                             # the smallest shape gf_lsop_predict16_eligible refuses (nC > LSOP_RING_MAXC)


def _all_k(cells, step=1):
    return range(0, cells + 1, step)


def _low_relief(nr, nc):
    """a tile far below every ladder's S with the content of the plain families (one-byte residuals, no noise)"""
    return base_tile(nr, nc, 60.0).astype(np.int32)


def _heavy(nr, nc):
    """a tile far above every ladder's S (it is never packed: its content selects nothing)"""
    return ladder(nr, nc, noise_amp=200, seed=6)(nr * nc)


@functools.lru_cache(maxsize=None)
def huffman_plane(model):
    nr, nc = SMALL
    return build_family("huffman-plane-m%d" % model, "huffman", nr, nc, ladder(nr, nc, noise_amp=24), _all_k(nr * nc), MASKS[model],
                        extra=(_low_relief(nr, nc), _heavy(nr, nc)))


@functools.lru_cache(maxsize=None)
def huffman_flatplain(model):
    nr, nc = STRIP
    return build_family("huffman-flatplain-m%d" % model, "huffman", nr, nc, ladder(nr, nc, noise_amp=24), _all_k(nr * nc), MASKS[model],
                        extra=(_low_relief(nr, nc), _heavy(nr, nc)))


@functools.lru_cache(maxsize=None)
def huffman_wide(model):
    nr, nc = SMALL
    return build_family("huffman-wide-m%d" % model, "huffman", nr, nc, ladder(nr, nc, noise_amp=24, spikes=WIDE_SPIKES), _all_k(nr * nc), MASKS[model],
                        extra=(ladder(nr, nc, spikes=WIDE_SPIKES, base=base_tile(nr, nc, 60.0))(0), _heavy(nr, nc)))


@functools.lru_cache(maxsize=None)
def huffman_nulls():
    nr, nc = SMALL
    return build_family("huffman-nulls", "huffman", nr, nc, ladder(nr, nc, null_block=NULL_BLOCK), _all_k(nr * nc))


def rare_base(nr, nc, seed=0):
    """the tiles of test_encoder_pack_rare_receives_long_code_tiles: geometric row differences and two steps of 2^30"""
    rng = np.random.default_rng(nr + nc + seed)
    v = (rng.geometric(0.5, nr * nc) - 1).astype(np.int64).cumsum()
    v[(nr * nc) // 3:] += 2 ** 30
    v[2 * (nr * nc) // 3:] -= 2 ** 30
    return v


RARE_BITS = 64                                   # k_huffman_pack leaves a tile from here on: 2,048 cells x bits > (4,096 - 2) x 32
RARE_SHAPES = ((16, 40), (16, 64), (24, 50), (24, 64), (24, 100))


@functools.lru_cache(maxsize=None)
def huffman_rare():
    """the first shape of RARE_SHAPES at which every packing of the family is left to k_huffman_pack_rare (rare_bits >= RARE_BITS:
    the route report's word 5 then counts exactly the tiles that fit)"""
    for nr, nc in RARE_SHAPES:
        f = build_family("huffman-rare", "huffman", nr, nc, ladder(nr, nc, noise_amp=1, base=rare_base(nr, nc)), _all_k(nr * nc), 1)
        if all(rare_bits(nr, nc, f.tiles[t], 1) >= RARE_BITS for t in range(f.n) if f.packs[t] is not None):
            return f
    raise AssertionError("no shape of RARE_SHAPES sends every tile to k_huffman_pack_rare")


def general_shape():
    """a shape of k_huffman_encode<false> with two rows (the first of route_plan's sweep: tests/test_gpu_routes.py)"""
    import route_plan as rp
    return 2, rp.LEAN_MAX_CELLS // 2 + 1


GENERAL_K = (1000, 1032)                         # noise cells of the general family's two packed tiles (found once; asserted)


@functools.lru_cache(maxsize=None)
def huffman_general():
    """five tiles of about 1.4 M cells, two oracle encodes: S is the first multiple of 16 from the packing of GENERAL_K[0] noise
    cells on, and GENERAL_K[1] noise cells give a packing within 16 bytes over S"""
    nr, nc = general_shape()
    tile_of = ladder(nr, nc, noise_amp=3)
    f = Family("huffman-general", "huffman", nr, nc, 1)
    f.relaxed = True
    under, over = (tile_of(k) for k in GENERAL_K)
    p_under, p_over = (encode_one("huffman", nr, nc, v, 1) for v in (under, over))
    S = (len(p_under[0]) + 15) // 16 * 16
    assert S < len(p_over[0]) <= S + 16, (S, len(p_under[0]), len(p_over[0]))
    nulls = np.full(nr * nc, NULL, np.int32)
    for v, (pk, pred) in ((under, p_under), (nulls, (None, 0)), (over, p_over), (nulls, (None, 0)), (under, p_under)):
        f.tiles.append(v)
        f.packs.append(pk)
        f.preds.append(pred)
        f.lengths.append(len(pk) if pk is not None else 0)
    f.stride = S
    f.all_lengths = sorted(set(f.lengths))
    return f


def _uniform(nr, nc, value=77):
    return np.full(nr * nc, value, np.int32)


@functools.lru_cache(maxsize=None)
def canon_plain(model):
    nr, nc = SMALL
    return build_family("canon-plain-m%d" % model, "canon", nr, nc, ladder(nr, nc, noise_amp=24), _all_k(nr * nc), MASKS[model],
                        extra=(_uniform(nr, nc), _heavy(nr, nc)))


@functools.lru_cache(maxsize=None)
def canon_nulls():
    nr, nc = SMALL
    return build_family("canon-nulls", "canon", nr, nc, ladder(nr, nc, null_block=NULL_BLOCK), _all_k(nr * nc), extra=(_uniform(nr, nc), _heavy(nr, nc)))


UNIFORM_STRIDE = 16                              # the smallest slot_stride the ABI takes: slotWords = 4


@functools.lru_cache(maxsize=None)
def canon_uniform():
    """gvrs_canon_encode.hip, the uniform form (a tile of one value packs to 6 bytes, predictor 0), at the smallest legal stride:
    the uniform tiles are the only ones that fit, every varied tile -- plain, with escapes, with a block of nulls, for each
    predictor the oracle picks -- reports GF_OVERFLOW with its full length and all-null tiles are declined.  Every uniform tile
    is followed by a tile that writes nothing; one is the first tile and one the last."""
    nr, nc = SMALL
    f = Family("canon-uniform", "canon", nr, nc)
    f.stride = UNIFORM_STRIDE
    nulls = np.full(nr * nc, NULL, np.int32)
    varied = [ladder(nr, nc, noise_amp=24)(0), ladder(nr, nc)(nr * nc), ladder(nr, nc, null_block=NULL_BLOCK)(300),
              ladder(nr, nc, cells_set=escape_cells(nr, nc))(100), _low_relief(nr, nc), _heavy(nr, nc)]
    uniform = [_uniform(nr, nc, v) for v in (77, 0, -1, 2 ** 31 - 1, -2 ** 31 + 1, 12345678, -300)]
    tiles = []
    for i, u in enumerate(uniform):
        tiles += [u, nulls if i % 2 else varied[i % len(varied)]]
    tiles += varied + [nulls, uniform[0]]
    for v in tiles:
        pk, pred = encode_one("canon", nr, nc, v)
        f.tiles.append(v)
        f.packs.append(pk)
        f.preds.append(pred)
        f.lengths.append(len(pk) if pk is not None else 0)
    f.all_lengths = sorted(set(f.lengths))
    return f


def escape_cells(nr, nc):
    """class-edge values of every escape kind (value_edges.CANON_EDGES outside the gap, not the null code) as the values of cells
    spread over the tile"""
    vals = [e for e in ve.CANON_EDGES if not ve.in_gap(e) and e != NULL and ve.canon_kind(e) >= 1]
    step = (nr * nc - 8) // len(vals)
    return tuple((5 + i * step, v) for i, v in enumerate(vals))


@functools.lru_cache(maxsize=None)
def canon_escape():
    nr, nc = SMALL
    return build_family("canon-escape", "canon", nr, nc, ladder(nr, nc, cells_set=escape_cells(nr, nc)), _all_k(nr * nc), 1)


@functools.lru_cache(maxsize=None)
def lsop(wide, checksum):
    nr, nc = LSOP_WIDE if wide else SMALL
    assert lsop16_eligible(nr, nc) == (not wide)
    return build_family("lsop-%d%s" % (32 if wide else 16, "-checksum" if checksum else ""), "lsop", nr, nc, ladder(nr, nc),
                        _all_k(nr * nc), lsop_flags=LSOP_CHECKSUM if checksum else 0, lo=64)


LSOP08_ODD = (15, 41)                            # 615 cells: tile t of a batch starts 12 t bytes past a 16-byte boundary


@functools.lru_cache(maxsize=None)
def lsop08(wide):
    nr, nc = LSOP_WIDE if wide else LSOP08_ODD
    assert (nr * nc) % 4 != 0
    return build_family("lsop08-%s" % ("wide" if wide else "odd"), "lsop08", nr, nc, ladder(nr, nc), _all_k(nr * nc), lo=64)


@functools.lru_cache(maxsize=None)
def m32(edge=0):
    """sub_stride S such that the lengths S - 11 .. S - 7 occur among the streams of candidate `edge` (0 Differencing, 1 Linear;
    the rule is length + 8 <= S: S - 8 is the longest stream that is written, S - 7 the first that is not); one tile per length of
    that candidate within S - 8 +- NEAR, the ladder's two ends and two tiles with a block of nulls.
    edge 0: the Linear stream behind every Differencing stream at the edge is longer and stays unwritten -- whatever the packer
    wrote past the Differencing stream's sub-slot stays visible.  edge 1: Differencing and Triangle streams are written around
    the Linear stream at the edge (a candidate that does not fit between two that do)."""
    nr, nc = SMALL
    tile_of = ladder(nr, nc)
    cand = {k: m32_candidate_lengths(nr, nc, tile_of(k)) for k in _all_k(nr * nc)}
    lens = [c[edge] for c in cand.values()]
    S = pick_stride([L + 8 for L in lens], 16, (-3, -2, -1, 0, 1))
    assert S is not None
    f = Family("m32-%s" % ("differencing", "linear")[edge], "m32", nr, nc)
    f.stride = S
    f.all_lengths = sorted(set(lens))
    by_len = {}
    for k in sorted(cand):
        by_len.setdefault(cand[k][edge], k)
    ks = [0, nr * nc] + sorted({by_len[L] for L in by_len if abs(L + 8 - S) <= NEAR}) + [0, nr * nc]
    tiles = [tile_of(k) for k in ks]
    with_nulls = ladder(nr, nc, null_block=NULL_BLOCK)
    tiles[2:2] = [with_nulls(0)]
    tiles.append(with_nulls(nr * nc))
    for v in tiles:
        streams, models, seed = m32_candidates(nr, nc, v)
        f.tiles.append(v)
        f.packs.append(streams)
        f.preds.append(models)
        f.lengths.append(tuple(len(s) if s is not None else 0 for s in streams))
        f.seeds.append(seed)
    return f


SMALL_FAMILIES = ([(huffman_plane, (m,)) for m in (1, 2, 3)] + [(huffman_flatplain, (m,)) for m in (1, 2, 3)]
                  + [(huffman_wide, (m,)) for m in (1, 2, 3)] + [(huffman_nulls, ()), (huffman_rare, ())]
                  + [(canon_plain, (m,)) for m in (1, 2, 3)] + [(canon_nulls, ()), (canon_escape, ())]
                  + [(lsop, (w, c)) for w in (False, True) for c in (False, True)] + [(lsop08, (w,)) for w in (False, True)])


def family_id(entry):
    fn, args = entry
    return fn.__name__ + "".join("-%s" % (int(a) if isinstance(a, bool) else a) for a in args)


# ---- hand-made slots for gf_compact_dev

COMPACT_STRIDE = 48
COMPACT_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 47, 48)


def compact_order():
    """the lengths of COMPACT_LENGTHS, each four times, in an order in which short tiles (less than 8 bytes: no whole aligned word
    on most alignments) and long ones each start at every destination misalignment 0 .. 3 (found greedily; asserted)"""
    pool = [L for L in COMPACT_LENGTHS for _ in range(4)]
    order, off = [], 0
    need = {(short, m) for short in (True, False) for m in range(4)}
    while need:
        pick = next((L for L in pool if L > 0 and (L < 8, off % 4) in need), None)
        if pick is None:
            pick = next(L for L in pool if L % 4 in (1, 3))       # shift the alignment
        else:
            need.discard((pick < 8, off % 4))
        pool.remove(pick)
        order.append(pick)
        off += pick
    return order + pool


def compact_slots(lengths, stride=COMPACT_STRIDE, seed=11):
    """(slots [n, stride] of known bytes -- the sentinel behind each packing --, the concatenation)"""
    rng = np.random.default_rng(seed)
    slots = np.full((len(lengths), stride), SENTINEL, np.uint8)
    for t, L in enumerate(lengths):
        slots[t, :L] = rng.integers(0, 256, L)
        slots[t, :L][slots[t, :L] == SENTINEL] = 0x11
    cat = b"".join(slots[t, :L].tobytes() for t, L in enumerate(lengths))
    return slots, cat
