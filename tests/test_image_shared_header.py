"""CPU-only: gridfour_amd/csrc/gvrs_image_common.h, the restatement of the reference's image loops that the kernels inline --
split, join and the packed-word accumulator of the reduce -- compiled with g++ into a program of its own
(tests/csrc/image_harness.cpp) and compared BIT FOR BIT with the numpy model of tests/image_ref.py on random words, on the edge
values of the join and on windows at the rounding boundary of the reduce.  The same program built with
-fsanitize=address,undefined runs the same kinds of input once more, directly."""
import numpy as np
import pytest

import image_cases as K
import image_ref as M


@pytest.fixture(scope="module")
def ih():
    return K.build_harness()


def _split_join(exe, tmp, n, seed):
    rng = np.random.default_rng(seed)
    w = K.random_words(rng, n)
    w[:4] = (0xff102030, 0x00ff0000, 0x00ffffff, 0)
    for model in M.MODELS:
        want = M.split(model, w)
        got = K.harness_split(exe, tmp, model, w)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), model
        assert np.array_equal(K.harness_join(exe, tmp, model, got).view(np.uint32), w | np.uint32(0xff000000)), model
        for elem_type, fill in ((M.INT, M.INT_MIN), (M.INT, 12345), (M.SHORT, -32768)):
            planes = K.join_planes(rng, n, fill, elem_type)
            assert np.array_equal(K.harness_join(exe, tmp, model, planes), M.join(model, planes)), (model, elem_type)
        edge = [np.array([v], np.int32) for v in (M.INT_MIN,) * 3]
        assert K.harness_join(exe, tmp, model, edge).view(np.uint32).tolist() == [0xff000000]


def _reduce(exe, tmp, factors, seed):
    rng = np.random.default_rng(seed)
    for f in factors:
        img = K.boundary_image(f, 5, 7, rng)
        want = M.reduce(img, f)
        assert want.shape == (5, 7)
        assert np.array_equal(K.harness_reduce(exe, tmp, img, f), want), f
    white = np.full((9, 11), 0x00ffffff, np.uint32)
    assert (K.harness_reduce(exe, tmp, white, 4).view(np.uint32) == 0xffffffff).all()
    assert K.harness_reduce(exe, tmp, white, 10).shape == (0, 1)


def test_split_and_join_equal_the_model(ih, tmp_path):
    _split_join(ih, str(tmp_path), 5000, 10)


def test_reduce_equals_the_model(ih, tmp_path):
    _reduce(ih, str(tmp_path), K.REDUCE_FACTORS, 20)


def test_the_largest_factor_does_not_wrap(ih, tmp_path):
    """one all-white window of 2899 x 2899 pixels: 2899^2 * 255 + 2899^2 / 2 is the largest sum the accumulator meets"""
    f = M.MAX_FACTOR
    white = np.full((f, f), 0xffffffff, np.uint32)
    assert K.harness_reduce(ih, str(tmp_path), white, f).view(np.uint32).tolist() == [[0xffffffff]]


def test_under_the_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined, run directly: a report ends it with a non-zero status"""
    exe = K.build_harness(("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"), "image_harness_san")
    _split_join(exe, str(tmp_path), 600, 30)
    _reduce(exe, str(tmp_path), (1, 2, 3, 8, 9), 40)
