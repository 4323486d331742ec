"""The fast Huffman decoder's subsequence synchronisation on tiles where a subsequence start can go wrong.

k_huffman_decode<FAST> cuts a tile's text into subsequences of `unit` bits, starts each one a warm-up stretch in front of its
boundary and decodes again, from the predecessor's end, those whose start turned out wrong (fast_sync_pass in
csrc/gvrs_decode.hip).  The redo rounds are exact, so the warm-up length and the shape of the decode loop can only change speed --
as long as wrong starts are found and repaired.  The contents here are chosen because starts do go wrong on them, or because
the text sits at an edge of the subsequence grid:

* periodic text (a two-value checkerboard, stripes of period 3): any phase of the period parses, a wrong start can stay wrong;
* a DEM tile with a flat lower half: one-bit codes for half the text, a warm-up of many symbols;
* a few rare symbols among thousands of common ones: codes longer than the 10-bit window, and beyond 18 bits (both lookup
  levels) where the tile has the cells for such a tree;
* a constant tile (a tree of a single leaf: no text);
* tiny tiles, whose text is shorter than the warm-up and shorter than one unit;
* 120 x 150 tiles whose last values were flattened until the text ends within a code of a multiple of `unit`.

Every case is 8 tiles, through the host batch and the device-resident batch entry points: the device's packing equals the
oracle's, the device's decode of the oracle's packing equals the values, every status is 0.  One shape per thread build of the
decoder -- 32 x 48 (256 threads), 120 x 150 (512), 167 x 167 (1,024: the first square the route plan gives that build) --, and
every case asserts, through the route plan and the route report, that this build of the fast kernel is the one that ran."""
import os
import subprocess
import sys

import numpy as np
import pytest

import damage as D
import oracle
import route_plan as rp

pytestmark = pytest.mark.gpu
N = 8
SHAPES = [(32, 48), (120, 150), (167, 167)]
BUILD = {(32, 48): 256, (120, 150): 512, (167, 167): 1024}        # threads of the decoder build the route plan picks
TINY = [(2, 2), (3, 5), (8, 8)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_codec = []


def _hip():
    import gridfour_amd
    if not _codec:
        _codec.append(gridfour_amd.CodecHuffmanHip(device=0))
    return gridfour_amd, _codec[0]


def checkerboards(r, c, n=N):
    i, j = np.mgrid[0:r, 0:c]
    return np.stack([(100 * k - 300 + ((i + j) & 1) * (1 + 3 * k)).ravel() for k in range(n)]).astype(np.int32)


def stripes3(r, c, n=N):
    """period 3 along the columns, along the rows and along the diagonal, three values each"""
    i, j = np.mgrid[0:r, 0:c]
    out = []
    for k in range(n):
        phase = (j, i, i + j, 2 * i + j)[k % 4] % 3
        levels = np.array([0, 1 + k, 5 + 2 * k], np.int32)
        out.append((levels[phase] + 50 * k).ravel())
    return np.stack(out).astype(np.int32)


def periodic(r, c):
    return np.concatenate([checkerboards(r, c, N // 2), stripes3(r, c, N // 2)])


def dem_flat_half(r, c):
    v = oracle.dem_tiles(oracle.DEM_SEED + 41, r, c, 64, 0, N).reshape(N, r, c).copy()
    for k in range(N):
        v[k, r // 2:, :] = v[k, r // 2, 0]
    return v.reshape(N, r * c)


def rare_symbols(r, c):
    """differences with Fibonacci counts, in the order of the Differencing predictor (along the rows, a row's first cell from the
    first cell of the row above): the rarest ones get the deepest codes a tile of this size can have; they are dealt out at
    random over the tile"""
    cells = r * c
    out = []
    for k in range(N):
        fib = [1, 1]
        while sum(fib) + fib[-1] + fib[-2] <= cells - 1:
            fib.append(fib[-1] + fib[-2])
        deltas = np.concatenate([np.full(cnt, (i + 1) // 2 * (1 if i & 1 else -1), np.int32) for i, cnt in enumerate(reversed(fib))])
        deltas = np.concatenate([[0], deltas, np.zeros(cells - 1 - deltas.size, np.int32)])
        np.random.default_rng(900 + k).shuffle(deltas[1:])
        d = deltas.reshape(r, c)
        first = 1000 + k + np.cumsum(d[:, 0])                     # the first column, row after row
        d[:, 0] = 0
        out.append((first[:, None] + np.cumsum(d, axis=1)).ravel())
    return np.stack(out).astype(np.int32)


def constant(r, c):
    return np.stack([np.full(r * c, 37 * k - 100, np.int32) for k in range(N)])


def tiny_mix(r, c):
    """what fits a tile of a few cells and leaves its text below one unit (128 bits): two values, three values, ramps, a few
    steps on flat ground, a constant"""
    rng = np.random.default_rng(r * 100 + c)
    i, j = np.mgrid[0:r, 0:c]
    ramps = np.stack([(2 * i + j + 7).ravel(), (40 - i - 3 * j).ravel()])
    steps = np.cumsum(rng.random((1, r * c)) < 0.15, axis=1) + 5
    return np.concatenate([checkerboards(r, c, 2), stripes3(r, c, 2), ramps, steps, constant(r, c)[:1]]).astype(np.int32)


def text_bits(pk):
    """the text as the kernel sees it: from the end of the tree to the end of the packing"""
    return len(pk) * 8 - D.huffman_tree_walk(pk)[0]


def unit_of(bits, max_q=512):
    """huffman_to_m32_fast: bits per subsequence (max_q = 512 subsequences in the 256- and 512-thread builds)"""
    return max(128, ((bits + max_q - 1) // max_q + 31) & ~31)


def trimmed_to_unit(r, c):
    """DEM tiles whose last j values repeat the one in front of them, j the first for which the text ends within eight bits (the
    packing ends on a byte; a code of terrain is about five bits) of a multiple of unit"""
    dem = oracle.dem_tiles(oracle.DEM_SEED + 47, r, c, 64, 0, N).reshape(N, r * c)
    out = []
    for k in range(N):
        for j in range(1, 400):
            v = dem[k].copy()
            v[-j:] = v[-j - 1]
            bits = text_bits(oracle.codec_huffman_encode(0, r, c, v)[0])
            rem = bits % unit_of(bits)
            if (rem <= 8 and k % 2 == 0) or (rem >= unit_of(bits) - 8 and k % 2 == 1):      # just behind / just in front of a boundary
                out.append(v)
                break
        else:
            raise AssertionError("no trim of tile %d brings its text to a subsequence boundary" % k)
    return np.stack(out)


def _check(r, c, tiles, build=None):
    """the four properties of the module docstring, through the host batch and the device-resident batch"""
    gridfour_amd, codec = _hip()
    tiles = np.ascontiguousarray(tiles, np.int32).reshape(N, r * c)
    ref = [oracle.codec_huffman_encode(0, r, c, tiles[t])[0] for t in range(N)]
    assert all(p is not None for p in ref), "the oracle declines a tile of this case"
    # host batch
    packs, _, status = codec.encode_batch(0, r, c, tiles)
    assert (np.asarray(status) == 0).all(), status
    assert [bytes(p) for p in packs] == [bytes(p) for p in ref]
    vals, st = codec.decode_batch(r, c, ref)
    assert (np.asarray(st) == 0).all(), st
    assert np.array_equal(np.asarray(vals).reshape(N, r * c), tiles)
    # device-resident batch
    b = gridfour_amd.DeviceTileBatch(codec.ctx, r, c, N, slot_stride=(2 * r * c + 1024 + 15) // 16 * 16)
    try:
        b.values.upload(tiles)
        b.encode()
        assert (b.get_enc_status() == 0).all()
        assert [b.get_packing(t) for t in range(N)] == [bytes(p) for p in ref]
        _load_packings(b, ref)
        b.decoded.fill(0xA5)
        b.decode()
        assert (b.get_dec_status() == 0).all()
        assert np.array_equal(b.get_decoded(), tiles)
        if build is not None:
            # the fast kernel of the build this shape stands for is what the batch launched
            assert rp.plan(rp.KIND_HUFFMAN, r, c, N).decThreads == build
            assert rp.report(codec.ctx).decBits & rp.dec_bit(rp.DEC_FAST, build), (build, hex(rp.report(codec.ctx).decBits))
    finally:
        b.free()


def _load_packings(b, packs):
    slots = np.full(b.n_tiles * b.stride, 0xA5, np.uint8)
    for t, p in enumerate(packs):
        slots[t * b.stride:t * b.stride + len(p)] = np.frombuffer(bytes(p), np.uint8)
    b.slots.upload(slots)
    b.lengths.upload(np.array([len(p) for p in packs], np.uint32))


@pytest.mark.parametrize("content", [periodic, dem_flat_half, rare_symbols, constant], ids=lambda f: f.__name__)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_resync_contents(shape, content):
    r, c = shape
    tiles = content(r, c)
    if content is rare_symbols:
        # the tree really is deeper than the window, and than both lookup levels where the cells allow (Fibonacci counts: depth d
        # needs about 1.6^d cells)
        deepest = min(D.huffman_tree_walk(oracle.codec_huffman_encode(0, r, c, t)[0])[1] for t in tiles)
        assert deepest > (18 if r * c >= 18000 else 10), deepest
    _check(r, c, tiles, BUILD[shape])


@pytest.mark.parametrize("shape", TINY, ids=lambda s: "%dx%d" % s)
def test_resync_tiny_tiles(shape):
    r, c = shape
    tiles = tiny_mix(r, c)
    for t in tiles:
        pk = oracle.codec_huffman_encode(0, r, c, t)[0]
        assert pk is not None and text_bits(pk) < 128          # shorter than one unit, which is at least 128 bits
    _check(r, c, tiles)


def test_resync_text_ends_at_a_unit_boundary():
    r, c = 120, 150
    tiles = trimmed_to_unit(r, c)
    for k, t in enumerate(tiles):
        bits = text_bits(oracle.codec_huffman_encode(0, r, c, t)[0])
        rem = bits % unit_of(bits)
        assert rem <= 8 or rem >= unit_of(bits) - 8, (k, bits, rem)
    _check(r, c, tiles, BUILD[(r, c)])


_ROUNDS_SCRIPT = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import gridfour_amd, oracle
from gridfour_amd import DeviceBuffer, DeviceTileBatch, lib
import test_gpu_decode_resync as T
r, c, n = 120, 150, T.N
tiles = T.periodic(r, c)
ctx = gridfour_amd.GvrsHipContext(0)
b = DeviceTileBatch(ctx, r, c, n, slot_stride=(2 * r * c + 1024 + 15) // 16 * 16)
T._load_packings(b, [oracle.codec_huffman_encode(0, r, c, t)[0] for t in tiles])
L = lib(); L.gf_internal_set_decode_debug.argtypes = [C.c_void_p]
dbg = DeviceBuffer(ctx, 16 * 4 * n).fill(0)
L.gf_internal_set_decode_debug(dbg.ptr)
b.decode(); ctx.synchronize()
L.gf_internal_set_decode_debug(None)
st = dbg.download(np.uint32, 16 * n).reshape(n, 16)
ok = (b.get_dec_status() == 0).all() and np.array_equal(b.get_decoded(), tiles)
print("ROUNDS", " ".join(str(int(x)) for x in st[:, 11]), "LISTED", " ".join(str(int(x)) for x in st[:, 9]), "OK", int(ok))
"""


def test_periodic_tiles_take_more_than_one_round():
    """the diagnostic library's per-tile record (GF_DIAG: word 11 = rounds of the synchronisation pass, word 9 = subsequences
    redone): some periodic tile starts a subsequence wrong and needs a redo round -- else the cases above do not test one.  The
    diagnostic library is a process-wide choice, so this runs in a process of its own; it is not built by default."""
    from gridfour_amd import build
    if not os.path.exists(build.LIB_DIAG) or build.needs_build(build.LIB_DIAG):
        pytest.skip("the diagnostic library (GF_DIAG) is not built")
    env = dict(os.environ, GVRS_HIP_DIAG="1")
    env.pop("GVRS_HIP_VARIANT", None)
    out = subprocess.run([sys.executable, "-c", _ROUNDS_SCRIPT, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("ROUNDS")][-1].split()
    rounds = [int(x) for x in line[1:line.index("LISTED")]]
    listed = [int(x) for x in line[line.index("LISTED") + 1:line.index("OK")]]
    assert line[-1] == "1", "the diagnostic build decodes the periodic tiles wrong"
    assert max(rounds) > 1 and max(listed) > 0, (rounds, listed)
