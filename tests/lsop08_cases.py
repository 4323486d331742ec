"""Tiles and containers that drive the LSOP08 kernels (gvrs_lsop8.hip) into the branches tests/test_gpu_lsop08_shapes.py and
tests/test_gpu_lsop08_pack.py are about, built with the restatement (tests/lsop08_ref.py) alone.  The property each one is built for
is proved on the CPU in tests/test_lsop08_ref.py; the GPU tests assert it again where it is cheap.

  threshold_tiles   tiles one unit either side of the predictor's switch between exact sums and scan-order sums
  overflow_tile     a tile with a chunk of 1,024 interior values whose codes exceed the packer's 2,048-word window
  single_symbol_*   tiles and containers whose Huffman segments take the single-symbol form (17 tree bits, no text)
  max_body_tiles    tiles that make the body of a packing as long as a tile of their shape can"""
import functools
import math

import numpy as np

import lsop08_ref as R

TWO53 = 2 ** 53
WINDOW_BITS = 2048 * 32                      # P8_WIN_WORDS * 32 (gvrs_lsop8.hip)
MAX_CODE_BITS = 56                           # the longest code k_lsop8_pack strings together


# ---- the exact / scan-order switch
def largest_exact_magnitude(n_int):
    """the largest integer m with m * m * n_int < 2^53"""
    m = math.isqrt((TWO53 - 1) // n_int)
    assert m * m * n_int < TWO53 <= (m + 1) * (m + 1) * n_int
    return m


def bound(nr, nc, v):
    """max|v|^2 * interior cells, as Python integers: k_lsop8_predict sums exactly where this is below 2^53"""
    m = max(abs(int(x)) for x in v)
    return m * m * R.n_interior(nr, nc)


@functools.lru_cache(maxsize=None)
def threshold_tiles(nr, nc):
    """{name: tile}: `at-<where>` holds the largest exact magnitude m once, at an interior cell (`mid`), in row 0 (`row0`) or in the
    last cell (`last`), every other value random in [-m, m]; `over-<where>` is the same tile with that cell at m + 1; `int32min`
    holds INT32_MIN.  Every tile is one the restatement does not decline (the seed is searched)."""
    m = largest_exact_magnitude(R.n_interior(nr, nc))
    cells = nr * nc
    where = {"mid": (nr // 2) * nc + nc // 2, "row0": nc // 2, "last": cells - 1}
    out = {}
    for name, cell in where.items():
        for seed in range(50):
            v = np.random.default_rng(1000 * seed + cells + cell).integers(-m, m + 1, cells)
            v[cell] = m
            over = v.copy()
            over[cell] = m + 1
            if R.coefficients(nr, nc, v) is not None and R.coefficients(nr, nc, over) is not None:
                break
        else:
            raise AssertionError("no tile of %d x %d that is not declined" % (nr, nc))
        out["at-" + name], out["over-" + name] = v.astype(np.int32), over.astype(np.int32)
    for seed in range(50):
        v = np.random.default_rng(77 + seed).integers(-m, m + 1, cells)
        v[where["mid"]] = R.I32_MIN
        if R.coefficients(nr, nc, v) is not None:
            break
    else:
        raise AssertionError("no tile with INT32_MIN that is not declined")
    out["int32min"] = v.astype(np.int32)
    return out


# ---- the packer's window
OVERFLOW_MAX_CELLS = 2 ** 21
# (side, noise rows) in the order tried: the four rows at 1,024 x 1,024 first; fewer noise values among as many low-relief ones make
# the noise bytes' codes longer, so one row from there on, the side growing in steps of 128 as far as OVERFLOW_MAX_CELLS allows
OVERFLOW_CANDIDATES = [(1024, 4)] + [(n, 1) for n in range(1024, 1449, 128)]
# What a chunk must exceed the window by: 1.5 KiB.  A packer that sent a chunk a few words over the window through the window all
# the same would still write the right bytes: behind the window lie its four spare words and 56 bytes of the shared block that hold
# nothing the text loop still needs, then whatever padding the LDS allocation has.  1.5 KiB is more than those together (an
# allocation is padded to 1,280 bytes at most): such a chunk runs out of the workgroup's LDS, where the CDNA instruction set drops
# stores and answers loads with 0, and the packing misses those codes.
OVERFLOW_MARGIN_BITS = 1536 * 8


def low_relief_with_noise_rows(n, rows, seed=3):
    """an n x n tile of low relief with `rows` rows of 32-bit noise, one in each of as many bands of the tile: the row of the band
    whose interior values begin nearest a multiple of 1,024 in the stream, so that one chunk holds (nearly) nothing else"""
    rng = np.random.default_rng(seed + n)
    r, c = np.mgrid[0:n, 0:n]
    v = (np.rint(40 * np.sin(r / 60.0) * np.cos(c / 45.0)) + rng.integers(-2, 3, (n, n))).astype(np.int64)
    for k in range(rows):
        band = range(k * n // rows + 8, (k + 1) * n // rows - 8)
        v[min(band, key=lambda q: (((q - 2) * (n - 2)) % R.CHUNK, q))] = rng.integers(-2 ** 31 + 1, 2 ** 31, n)
    return v.astype(np.int32).ravel()


class Overflow:
    """tile, its type-0 packing and what the CPU found: side, noise rows, the interior stream's chunk bits, the longest code of each
    segment, and (side, rows, largest chunk, smallest chunk) of every candidate tried"""


@functools.lru_cache(maxsize=None)
def overflow_tile():
    """the first of OVERFLOW_CANDIDATES at which one chunk of the interior stream has OVERFLOW_MARGIN_BITS more code bits than the
    window holds and another fewer than the window less a chunk's lead (31 bits at most)"""
    tried = []
    for n, rows in OVERFLOW_CANDIDATES:
        assert n * n <= OVERFLOW_MAX_CELLS
        v = low_relief_with_noise_rows(n, rows)
        pr = R.predict(n, n, v)
        assert pr is not None
        seed, u, init, inter = pr
        cl0, cl1 = R.segment_code_lengths(init)[0], R.segment_code_lengths(inter)[0]
        bits = R.chunk_bits(inter, cl1)
        tried.append((n, rows, max(bits), min(bits)))
        if max(bits) > WINDOW_BITS + OVERFLOW_MARGIN_BITS and min(bits) < WINDOW_BITS - 31:
            o = Overflow()
            o.side, o.rows, o.tile, o.chunk_bits, o.max_code = n, rows, v, bits, (int(cl0.max()), int(cl1.max()))
            o.pack = R.container(6, seed, u, init, inter, R.TYPE_HUFFMAN)[0]
            o.tried = tried
            return o
    raise AssertionError("no tile up to 2^21 cells has a chunk far enough beyond the window: (side, rows, largest, smallest chunk) %r" % (tried,))


# ---- single-symbol segments
def distinct_bytes(stream):
    return len(set(R.m32_seq(stream)))


@functools.lru_cache(maxsize=None)
def single_symbol_first(nr=9, nc=11):
    """a tile whose rows 0, 1 and columns 0, 1 hold one value and whose interior is random: every initialiser is 0, so the first
    segment holds one symbol"""
    for seed in range(50):
        g = np.full((nr, nc), 41, np.int64)
        g[2:, 2:] = np.random.default_rng(900 + seed).integers(-300, 301, (nr - 2, nc - 2))
        v = g.astype(np.int32).ravel()
        if R.predict(nr, nc, v) is not None:
            return nr, nc, v
    raise AssertionError("every tile was declined")


SECOND_SEARCH_SEEDS = 400


@functools.lru_cache(maxsize=None)
def single_symbol_second():
    """(nr, nc, tile, seed) of the first seeded low-amplitude tile from 5 x 5 to 8 x 8 that is not declined and whose interior M32 bytes
    are all equal, or None where SECOND_SEARCH_SEEDS seeds a shape give none"""
    for n in (5, 6, 7, 8):
        for seed in range(SECOND_SEARCH_SEEDS):
            v = np.random.default_rng(5000 * n + seed).integers(-4, 5, n * n).astype(np.int32)
            pr = R.predict(n, n, v)
            if pr is not None and distinct_bytes(pr[3]) == 1 and distinct_bytes(pr[2]) > 1:
                return n, n, v, seed
    return None


def single_symbol_containers(nr=6, nc=7, codec_index=4):
    """[(name, packing, tile)]: type-0 containers built from streams, with the first, the second and both segments of one symbol, in
    both header revisions; the tile is what the restatement reconstructs from the streams"""
    rng = np.random.default_rng(61)
    ni, nx = R.n_init(nr, nc), R.n_interior(nr, nc)
    u = R.COEF_SETS["dense"]
    varied = lambda n: rng.integers(-2000, 2001, n).tolist()
    cases = {"first": ([0] * ni, varied(nx)), "second": (varied(ni), [5] * nx), "both": ([-3] * ni, [7] * nx)}
    out = []
    for name, (init, inter) in cases.items():
        assert (distinct_bytes(init) == 1) == (name != "second") and (distinct_bytes(inter) == 1) == (name != "first")
        p = R.container(codec_index, 19, u, init, inter, R.TYPE_HUFFMAN)[0]
        want = R.reconstruct(nr, nc, 19, init, inter, u)
        out += [(name, p, want), (name + "-legacy", R.to_legacy_header(p), want)]
    return out


# ---- the longest bodies
MAX_BODY_SHAPES = [(4, 4), (7, 9), (33, 65), (6, 257)]


@functools.lru_cache(maxsize=None)
def max_body_tiles(nr, nc):
    """{name: tile}: `noise32`, uniform 32-bit noise (every residual five or six M32 bytes of any value), and `bytes`, the tile
    among 40 seeds of such noise whose two segments hold the most distinct M32 bytes -- all 256 in the interior's at 33 x 65, in both
    at 6 x 257, whose initialisers are enough bytes for that (tests/test_lsop08_ref.py asserts it): a serialised tree of 256 leaves
    is the largest there is"""
    from tilegen import make_tile
    best, best_n = None, (-1, -1)
    for seed in range(40):
        v = np.random.default_rng(31 * seed + nr * nc).integers(-2 ** 31 + 1, 2 ** 31, nr * nc).astype(np.int32)
        pr = R.predict(nr, nc, v)
        if pr is None:
            continue
        n = (min(distinct_bytes(pr[2]), distinct_bytes(pr[3])), distinct_bytes(pr[2]) + distinct_bytes(pr[3]))
        if n > best_n:
            best, best_n = v, n
        if n == (256, 512):
            break
    assert best is not None
    return {"noise32": make_tile("noise32", nr, nc), "bytes": best}
