"""The routes of k_lsop8_pack (gvrs_lsop8.hip) that a terrain tile does not take, byte for byte against tests/lsop08_ref.py: a chunk
of 1,024 values whose codes exceed the 2,048-word LDS window and are ORed into the packing directly; segments of one symbol (17
tree bits, no text), written and read; slots of exactly gf_lsop08_max_packing bytes under the longest bodies a shape can have.
The tiles are those of tests/lsop08_cases.py, whose properties tests/test_lsop08_ref.py proves on the CPU.  (Slots that are too
small, and what lies around a slot: tests/test_gpu_encode_bounds.py, family lsop08.)"""
import numpy as np
import pytest

import lsop08_cases as K
import lsop08_ref as R

pytestmark = pytest.mark.gpu

OK = 0
ids = lambda s: "%dx%d" % s


@pytest.fixture(scope="module")
def codec():
    import gridfour_amd
    return gridfour_amd.LsCodec08Hip()


@pytest.fixture(scope="module")
def overflow():
    """the tile and its packing, built once (about 6 s of CPU; the GPU work is one tile)"""
    return K.overflow_tile()


def test_chunk_beyond_the_window(codec, overflow):
    o = overflow
    n = o.side
    beyond = [b for b in o.chunk_bits if b > K.WINDOW_BITS]
    print("side %d, chunks beyond the window %d of %d, largest %d bits" % (n, len(beyond), len(o.chunk_bits), max(o.chunk_bits)))
    assert n * n <= K.OVERFLOW_MAX_CELLS and max(beyond) > K.WINDOW_BITS + K.OVERFLOW_MARGIN_BITS and min(o.chunk_bits) < K.WINDOW_BITS - 31
    assert max(o.max_code) <= K.MAX_CODE_BITS
    packs, st = codec.encode_batch_dev(6, n, n, o.tile[None, :])
    assert st[0] == OK and len(packs[0]) == len(o.pack), (st[0], len(packs[0] or b""), len(o.pack))
    if packs[0] != o.pack:
        a, b = np.frombuffer(packs[0], np.uint8), np.frombuffer(o.pack, np.uint8)
        bad = np.nonzero(a != b)[0]
        raise AssertionError("%d bytes differ, the first at %r" % (bad.size, bad[:8].tolist()))
    vals, st = codec.decode_batch_dev(n, n, [o.pack])
    assert st[0] == OK and np.array_equal(vals[0], o.tile)


def test_single_symbol_segments_written(codec):
    """encode side: every initialiser 0 (the first segment holds one symbol), and the interior's M32 bytes all equal (the second).
    The second tile is the first hit of a seeded search over 5 x 5 .. 8 x 8 tiles (lsop08_cases.single_symbol_second: 5 x 5, seed 250)."""
    nr, nc, v = K.single_symbol_first()
    seed, u, init, inter = R.predict(nr, nc, v)
    assert K.distinct_bytes(init) == 1 and K.distinct_bytes(inter) > 1
    found = K.single_symbol_second()
    assert found is not None
    nr2, nc2, v2, _ = found
    pr2 = R.predict(nr2, nc2, v2)
    assert K.distinct_bytes(pr2[3]) == 1 and K.distinct_bytes(pr2[2]) > 1
    for (r, c, tile, pr) in ((nr, nc, v, (seed, u, init, inter)), (nr2, nc2, v2, pr2)):
        want = R.container(3, *pr, ctype=0)[0]
        packs, st = codec.encode_batch_dev(3, r, c, np.stack([tile, tile]))
        assert st.tolist() == [OK, OK] and packs[0] == want and packs[1] == want, (r, c, len(packs[0] or b""), len(want))
        vals, st = codec.decode_batch_dev(r, c, [want, R.to_legacy_header(want)])
        assert (st == OK).all() and np.array_equal(vals[0], tile) and np.array_equal(vals[1], tile)


def test_single_symbol_segments_read(codec):
    """decode side: containers built from streams with the first, the second and both segments of one symbol, both header revisions,
    through the host form and the device form"""
    nr, nc = 6, 7
    cases = K.single_symbol_containers(nr, nc)
    assert [name for name, _, _ in cases] == ["first", "first-legacy", "second", "second-legacy", "both", "both-legacy"]
    packs = [p for _, p, _ in cases]
    for vals, st in (codec.decode_batch(nr, nc, packs), codec.decode_batch_dev(nr, nc, packs)):
        for t, (name, _, want) in enumerate(cases):
            assert st[t] == OK and np.array_equal(vals[t], want), (name, st[t])


@pytest.mark.parametrize("shape", K.MAX_BODY_SHAPES, ids=ids)
def test_a_slot_of_max_packing_fits(codec, shape):
    """the header's "gf_lsop08_max_packing always fits": slots of exactly that size (encode_batch_dev's slot stride) take the longest
    bodies of the shape -- 32-bit noise, and the noise tile whose segments hold the most distinct M32 bytes"""
    import gridfour_amd
    nr, nc = shape
    cap = int(gridfour_amd.lib().gf_lsop08_max_packing(nr, nc))
    tiles = K.max_body_tiles(nr, nc)
    names = sorted(tiles)
    want = [R.encode(6, nr, nc, tiles[k], force_type=0)[0] for k in names]
    assert all(64 <= len(p) <= cap for p in want) and cap % 16 == 0
    packs, st = codec.encode_batch_dev(6, nr, nc, np.stack([tiles[k] for k in names]))
    for t, k in enumerate(names):
        assert st[t] == OK and packs[t] == want[t], (k, st[t], len(packs[t] or b""), len(want[t]))
