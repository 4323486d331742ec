"""CPU-only: tests/image_ref.py, the numpy model the image tests take their expectations from, pinned by words worked out by hand
from the reference's loops (ExperimentalImageStorage.java:242-256, :275-286; DemoCOG.java:735-770) and by the property the
reference relies on: split-then-join gives every colour back."""
import numpy as np

import image_ref as M


def _u(w):
    return np.asarray(w).view(np.uint32) if np.asarray(w).dtype == np.int32 else np.asarray(w, np.uint32)


def _join1(model, a, b, c):
    return int(_u(M.join(model, [np.array([a], np.int32), np.array([b], np.int32), np.array([c], np.int32)]))[0])


def test_split_by_hand():
    # 0xff102030: r, g, b = 16, 32, 48; Co = -32, tmp = 48 + (-32 >> 1) = 32, Cg = 0, Y = 32
    y, co, cg = M.split(M.YCOCG, np.array([0xff102030], np.uint32))
    assert (int(y[0]), int(co[0]), int(cg[0])) == (32, -32, 0)
    assert [int(p[0]) for p in M.split(M.RGB, np.array([0xff102030], np.uint32))] == [16, 32, 48]
    # r, g, b = 255, 0, 0: Co = 255, tmp = 0 + 127, Cg = -127, Y = 127 + (-127 >> 1) = 127 - 64
    y, co, cg = M.split(M.YCOCG, np.array([0x00ff0000], np.uint32))
    assert (int(y[0]), int(co[0]), int(cg[0])) == (63, 255, -127)


def test_alpha_does_not_matter():
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 1 << 24, 1000, dtype=np.uint32)
    for model in M.MODELS:
        want = M.split(model, rgb)
        for alpha in (0x00, 0x7f, 0x80, 0xff):
            got = M.split(model, rgb | np.uint32(alpha << 24))
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
    img = rgb[:900].reshape(30, 30)
    assert np.array_equal(M.reduce(img, 3), M.reduce(img | np.uint32(0xab000000), 3))


def test_join_by_hand():
    # r = 256: 0xff00 | 0x100 = 0xff00, the red byte is 0
    assert _join1(M.RGB, 256, 0x12, 0x34) == 0xff001234
    # r = -1: 0xff00 | -1 = -1, << 8 | g, << 8 | b = 0xffff0000 | g << 8 | b
    assert _join1(M.RGB, -1, 0x12, 0x34) == 0xffff1234
    # a green above its byte spills into red: g = 0x100 -> (0xff0000 | 0x100) << 8
    assert _join1(M.RGB, 0, 0x100, 0) == 0xff010000
    assert _join1(M.RGB, 16, 32, 48) == 0xff102030 and _join1(M.YCOCG, 32, -32, 0) == 0xff102030
    assert _join1(M.YCOCG, 63, 255, -127) == 0xffff0000


def test_int_min_joins():
    # RGB: 0xff00 | r = 0x8000ff00, << 8 = 0x00ff0000, | g = 0x80ff0000, << 8 = 0xff000000, | b = 0xff000000
    assert _join1(M.RGB, M.INT_MIN, M.INT_MIN, M.INT_MIN) == 0xff000000
    # YCoCg: Cg >> 1 = -2^30, tmp = -2^31 + 2^30 = -2^30, g = -2^31 - 2^30 -> 2^30, b = -2^30 + 2^30 = 0, r = INT_MIN;
    # 0x00ff0000 | 0x40000000 = 0x40ff0000, << 8 = 0xff000000, | 0
    assert _join1(M.YCOCG, M.INT_MIN, M.INT_MIN, M.INT_MIN) == 0xff000000


def _image(f, sums):
    """an f x f image whose channel sums are sums = (r, g, b): ones in the first pixels of each channel"""
    img = np.zeros(f * f, np.uint32)
    for shift, s in zip((16, 8, 0), sums):
        img[:s] |= np.uint32(1 << shift)
    return img.reshape(f, f)


def test_reduce_by_hand():
    # f = 2, n = 4: (2 + 2) / 4 = 1, (1 + 2) / 4 = 0
    assert _u(M.reduce(_image(2, (2, 1, 2)), 2)).tolist() == [[0xff010001]]
    # f = 3, n = 9: (4 + 4) / 9 = 0, (5 + 4) / 9 = 1
    assert _u(M.reduce(_image(3, (4, 5, 4)), 3)).tolist() == [[0xff000100]]
    white = np.full((5, 7), 0x00ffffff, np.uint32)
    assert (_u(M.reduce(white, 2)) == 0xffffffff).all() and M.reduce(white, 2).shape == (2, 3)
    assert M.reduce(white, 6).shape == (0, 1) and M.reduce_size(7, 5, 6) == (1, 0)


def test_split_then_join_is_the_identity_on_every_colour():
    rgb = np.arange(1 << 24, dtype=np.uint32)
    for model in M.MODELS:
        planes = M.split(model, rgb)
        assert all(-32768 <= int(p.min()) and int(p.max()) <= 32767 for p in planes)          # the planes fit a SHORT element
        assert np.array_equal(_u(M.join(model, planes)), rgb | np.uint32(0xff000000))
        assert np.array_equal(_u(M.join(model, [p.astype(np.int16) for p in planes])), rgb | np.uint32(0xff000000))
