"""The numpy restatement of CodecFloat (tests/float_ref.py) against the CPU oracle, bit for bit, at the shapes the GPU tests of
the plane kernels use: both sides of the 1,024-row seam of k_float_planes_decode, on either kernel path, several column trips
per row, and every short-plane and over-long-plane packing those tests feed the device."""
import numpy as np
import pytest

import float_ref
import oracle

SHAPES = [(1025, 1), (1025, 4), (2049, 3), (2050, 4), (1024, 8), (1023, 5), (7, 9), (10, 16), (3, 131), (2, 1028)]


def _tiles(n_rows, n_cols):
    rng = np.random.default_rng(n_rows * 4099 + n_cols)
    return [float_ref.random_bits(rng, n_rows, n_cols), float_ref.chain_bits(n_rows, n_cols)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_planes_and_packings_equal_the_oracle(shape):
    n_rows, n_cols = shape
    for bits in _tiles(n_rows, n_cols):
        assert np.array_equal(np.concatenate(float_ref.planes(n_rows, n_cols, bits)), oracle.float_planes_encode(n_rows, n_cols, bits))
        for level in (9, 6):
            pk = float_ref.encode_floats(3, n_rows, n_cols, bits, level)
            assert pk == oracle.codec_float_encode(3, n_rows, n_cols, bits, level=level)
        assert np.array_equal(float_ref.decode_floats(n_rows, n_cols, pk), bits)
        assert np.array_equal(oracle.codec_float_decode(n_rows, n_cols, pk), bits)


def test_the_chain_tile_has_no_zero_link():
    """What makes chain_bits a test of the carries: no column-0 delta of any mantissa plane is zero."""
    for n_rows, n_cols in ((2050, 4), (1025, 1)):
        pl = float_ref.planes(n_rows, n_cols, float_ref.chain_bits(n_rows, n_cols))
        for p in pl[2:]:
            assert (p.reshape(n_rows, n_cols)[1:, 0] != 0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_short_and_long_planes_equal_the_oracle(shape):
    """One scratch array for the five planes: a short plane keeps what the plane before left, a long one is cut at the room."""
    n_rows, n_cols = shape
    bits = float_ref.random_bits(np.random.default_rng(n_rows * 31 + n_cols), n_rows, n_cols)
    good = float_ref.encode_floats(3, n_rows, n_cols, bits, 6)
    short, long = float_ref.damaged_plane_packings(good)
    assert len(short) == 21 and len(long) == 5
    differs = 0
    for pk in short:
        want = oracle.codec_float_decode(n_rows, n_cols, pk)
        assert np.array_equal(float_ref.decode_floats(n_rows, n_cols, pk), want)
        differs += int(not np.array_equal(want, bits))
    assert differs >= len(short) - 2
    for pk in long:
        assert np.array_equal(oracle.codec_float_decode(n_rows, n_cols, pk), bits)
        assert np.array_equal(float_ref.decode_floats(n_rows, n_cols, pk), bits)


def test_damage_is_an_error_on_both_sides():
    n_rows, n_cols = 7, 9
    bits = float_ref.random_bits(np.random.default_rng(5), n_rows, n_cols)
    good = float_ref.encode_floats(3, n_rows, n_cols, bits, 6)
    flipped = bytearray(good)
    flipped[-1] ^= 0x10                                  # Adler-32 of the last stream
    for pk in (good[:len(good) // 2], good[:5], bytes(flipped)):
        with pytest.raises(IOError):
            oracle.codec_float_decode(n_rows, n_cols, pk)
        with pytest.raises(IOError):
            float_ref.decode_floats(n_rows, n_cols, pk)
