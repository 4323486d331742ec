"""CPU-only: the numpy model of the reference's colour palette and shaded relief (tests/render_ref.py) against known answers: the
reference's own assertion on OceanBasemap.cpt (ColorPaletteTableReaderTest.java:56-57) and values worked out by hand from
ColorPaletteTable.java, ColorPaletteRecordRGB.java, ColorPaletteRecordHSV.java, Arrays.binarySearch and Color.HSBtoRGB."""
import numpy as np

import render_cases as RC
import render_ref as M


def one(pal, z, shade=None, unlimited=False):
    return int(pal.argb([z], None if shade is None else [shade], unlimited)[0])


def test_the_references_palette_files():
    ocean, etopo = RC.model("ocean"), RC.model("etopo1")
    assert ocean.n == 12 and etopo.n == 41 and RC.model("categorical").n == 3
    assert one(ocean, 0.0) == 0xffc0c0c0                                  # the reference's own assertion
    assert ocean.get_range_min() == -11000.0 and ocean.get_range_max() == 8000.0
    assert one(ocean, -0.0) == 0xffffffff                                 # sorts below the key 0: range1 of the record -35 .. 0
    assert ocean.argb_for_null == 0 and etopo.argb_for_null == 0xff808080
    null = 0xff808080
    assert one(etopo, 0.0) == 0xff336600
    assert one(etopo, 8500.0) == 0xffffffff                               # top of the last record
    assert one(etopo, 8500.0000001) == null and one(etopo, -11000.5) == null
    assert one(etopo, np.nan) == null and one(etopo, np.inf) == null and one(etopo, -np.inf) == null
    assert one(etopo, -11000.0) == 0xff0a0079                             # the first key: 10 0 121
    cat = RC.model("categorical")
    assert [one(cat, z) for z in (1.0, 1.5, 2.0, 3.999, 4.0)] == [0xff4000c0, 0xff4000c0, 0xff0040ff, 0xff0080ff, 0xff0080ff]
    assert one(cat, 0.999) == 0xff808080 and one(cat, 4.001) == 0xff808080


def test_binary_search_is_javas():
    keys = np.array([-0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 2.0])
    z = np.array([-1.0, -0.0, 0.0, 0.5, 1.0, 2.0, 3.0, np.nan, np.inf, -np.inf])
    # 1.0: low 0 high 6 -> mid 3, equal bits: found at 3 (not the first, not the last of the run)
    assert M.binary_search(keys, z).tolist() == [-1, 0, 1, -3, 3, 6, -8, -8, -8, -1]
    assert M.binary_search(np.array([np.nan]), np.array([np.nan, 1.0])).tolist() == [0, -1]
    assert M.binary_search(np.array([0.0]), np.array([-0.0])).tolist() == [-1]
    assert M.binary_search(np.array([-0.0]), np.array([0.0])).tolist() == [-2]


def test_a_point_record_and_equal_keys():
    pal = RC.model("point_records")                                       # sorted: (-0.0, 0.5) (0.0, 0.25) (1, 1) (2, 2)
    assert pal.range0.tolist() == [0.0, 0.0, 1.0, 2.0] and np.signbit(pal.range0[0]) and not np.signbit(pal.range0[1])
    assert one(pal, 1.0) == 0xff000000 and one(pal, 2.0) == 0xff000000    # t is NaN: every channel 0
    assert one(pal, 1.5) == 0 and one(pal, -1e-300) == 0
    assert one(pal, -0.0) == 0xff010101                                   # found at the key -0.0
    assert one(pal, 0.0) == 0xff030303                                    # ... and at the key 0.0
    assert one(pal, 0.25) == 0xff040404 and one(pal, 0.3) == 0            # the record before the insertion point alone is asked
    two = RC.model("two_equal_keys")                                      # sorted, stably by range1: (5, 6) (5, 9)
    assert two.range1.tolist() == [6.0, 9.0]
    assert one(two, 5.0) == 0xff00ff00                                    # low 0 high 1 -> mid 0
    assert one(two, 5.5) == 0xff2000df                                    # record (5, 9), t = 0.125: r = (int) 32.375, b = (int) 223.625
    assert one(two, 9.0) == 0xffff0000 and one(two, 9.5) == 0xff808080


def test_the_sort_is_stable():
    recs = [(0.0, 1.0, "rgb", (k, 0, 0), (k, 0, 0)) for k in (7, 3, 9)]
    assert [r[3][0] for r in M.Palette(recs).source] == [7, 3, 9]
    recs = [(0.0, 1.0, "rgb", (1, 0, 0), (1, 0, 0)), (-0.0, 1.0, "rgb", (2, 0, 0), (2, 0, 0)), (0.0, 0.5, "rgb", (3, 0, 0), (3, 0, 0))]
    assert [r[3][0] for r in M.Palette(recs).source] == [2, 3, 1]


def test_normalised_tables_and_the_hinge():
    pal = RC.model("normalized")                                          # 7 records tiling 0 .. 1, input -250 .. 4000
    plain = M.Palette(RC.PALETTES["normalized"]()["records"], 0xffabcdef)
    z = np.array([-250.0, 0.0, 1875.0, 4000.0, -250.1, 4000.1])
    t = (z - (-250.0)) / (4000.0 - (-250.0))
    assert np.array_equal(pal.argb(z), plain.argb(t * (1.0 - 0.0) + 0.0))
    assert one(pal, -250.1) == 0xffabcdef and one(pal, 4000.1) == 0xffabcdef
    assert pal.get_range_min() == -250.0 and pal.get_range_max() == 4000.0
    hinge = RC.model("hinge")                                             # 8 records tiling -1 .. 1, the hinge at record 4
    assert hinge.hinge_index == 4
    plain = M.Palette(RC.PALETTES["hinge"]()["records"], 0xff010101)
    below, above = np.array([-8000.0, -4000.0, -1e-9, -8000.5]), np.array([0.0, 1250.0, 2500.0, 2500.5])
    assert np.array_equal(hinge.argb(below), plain.argb((below - -8000.0) / (0.0 - -8000.0) * (0.0 - -1.0) + -1.0))
    assert np.array_equal(hinge.argb(above), plain.argb((above - 0.0) / (2500.0 - 0.0) * (1.0 - 0.0) + 0.0))
    assert one(hinge, -8000.5) == 0xff010101 and one(hinge, 2500.5) == 0xff010101
    assert one(hinge, -4000.0) != one(hinge, 1250.0)


def test_unlimited_range():
    etopo = RC.model("etopo1")
    assert one(etopo, -20000.0, unlimited=True) == one(etopo, -11000.0) and one(etopo, 9e9, unlimited=True) == 0xffffffff
    assert one(etopo, np.inf, unlimited=True) == 0xffffffff and one(etopo, -np.inf, unlimited=True) == 0xff0a0079
    assert one(etopo, np.nan, unlimited=True) == 0xff808080
    assert one(etopo, -20000.0, 0.5, unlimited=True) == one(etopo, -11000.0, 0.5) != one(etopo, -11000.0)
    gaps = RC.model("gaps_256")
    assert one(gaps, 20.0, unlimited=True) == 0xff112233                  # record 130 is 15.625 .. 18.75, the next key 23.4375: a gap stays one
    # a normalised table compares the INPUT with the records' own range (:568): rangeMin / rangeMax are not the normalised ones
    pal = RC.model("normalized")
    assert one(pal, 2000.0, unlimited=True) == one(pal, 1.0) and one(pal, -3.0, unlimited=True) == one(pal, 0.0)


def test_shades_on_rgb_records():
    rng = np.random.default_rng(1)
    for name in ("etopo1", "ocean", "gaps_256"):
        pal = RC.model(name)
        z = RC.lookup_z(pal, rng, 500)
        assert np.array_equal(pal.argb(z, np.ones(z.size)), pal.argb(z))  # a shade of 1.0 is the unshaded form
    ocean = RC.model("ocean")
    assert one(ocean, 0.0, 0.0) == 0xff000000
    assert one(ocean, 0.0, 1.5) == (0xff000000 | (288 << 16) | (288 << 8) | 288) & 0xffffffff   # 192 * 1.5 = 288: the channels run into each other
    assert one(ocean, 0.0, np.nan) == 0xff000000
    assert one(ocean, 0.0, -1.0) == (0xff000000 | ((-191 & 0xffffffff) << 16) | ((-191 & 0xffffffff) << 8) | (-191 & 0xffffffff)) & 0xffffffff
    assert one(ocean, 9000.0, 0.5) == 0


def test_hsb_to_rgb():
    f = lambda h, s, v: int(M.hsb_to_rgb([h], [s], [v])[0])
    assert f(0.0, 1.0, 1.0) == 0xffff0000 and f(1.0 / 3.0, 1.0, 1.0) == 0xff00ff00 and f(2.0 / 3.0, 1.0, 1.0) == 0xff0000ff
    assert f(1.0, 1.0, 1.0) == 0xffff0000 and f(-1.0, 1.0, 1.0) == 0xffff0000 and f(0.5, 1.0, 1.0) == 0xff00ffff
    assert f(0.25, 0.0, 0.5) == 0xff808080 and f(np.nan, 0.0, 1.0) == 0xffffffff
    assert f(1.0 / 6.0, 1.0, 1.0) == 0xffffff00                           # float32(1/6) * 6 = 1.0f: case 1, f = 0
    assert f(-2.8e-10, 1.0, 1.0) == 0xff000000                            # hue - floor(hue) rounds to 1.0f, h = 6.0f: no case
    assert f(np.nan, 1.0, 1.0) == 0xffff0000                              # (int) NaN = 0: case 0, r = v, g = t = NaN -> 0, b = p = 0
    assert f(0.0, 1.0, 2.0) == 0xff000000 | (510 << 16)                   # brightness beyond 1


def test_hsv_records():
    pal = RC.model("hsv")
    assert pal.wrap_around.tolist() == [True, True, False, False, False, False, False, False]
    assert pal.d[:, 0].tolist()[:6] == [20.0, -20.0, 0.0, 10.0 + 1e-7, 180.0, 0.0]
    assert one(pal, -25.0) == int(M.hsb_to_rgb([np.float32(0.0 / 360.0)], [np.float32(0.7)], [np.float32(0.7)])[0])   # 350 + 10 = 360 -> not > 360 -> 1.0f
    assert one(pal, -37.5) == int(M.hsb_to_rgb([np.float32(355.0 / 360.0)], [np.float32(0.8)], [np.float32(0.55)])[0])
    assert one(pal, 7.5) == int(M.hsb_to_rgb([np.float32(355.0 / 360.0)], [np.float32(0.875)], [np.float32(0.4375)])[0])  # 10 - 15 = -5 -> 355
    assert one(pal, 10.0) == 0xffff0000                                   # hue exactly 360 -> 1.0f -> red
    assert one(pal, 19.999999) != one(pal, 20.0)
    assert one(pal, 20.0) == 0xff000000                                   # the hue just below zero: black
    assert one(pal, 45.0) == 0xff999999                                   # saturation 0: (int)(0.6f * 255 + 0.5)
    assert one(pal, 45.0, 0.5) == 0xff4d4d4d                              # the shade scales the value: (int)(0.3f * 255 + 0.5) = 77
    assert one(pal, 65.0) == 0xff7e4102                                   # the RGB record of the same table
    assert one(pal, 45.0, np.nan) == 0xff000000


def test_illumination():
    sun = (0.0, 0.6, 0.8)
    li = M.Light(-2.0, 2.0, sun, 0.25)
    assert M.shade([0.0], [0.0], li)[0] == 0.8 * (1 - 0.25) + 0.25        # a level surface: dot = nz * sun z
    assert M.shade([0.0], [-1e9], li)[0] == 0.25                          # dot < 0: ambient
    assert M.shade([np.nan], [0.0], li)[0] == 0.25 and M.shade([0.0], [np.nan], li)[0] == 0.25
    assert M.shade([np.inf], [0.0], li)[0] == 0.25                        # inf / inf: NaN
    level = M.Light(1.0, 1.0, (0.0, 0.0, 0.0), 0.3)
    assert M.shade([1.0], [2.0], level)[0] == 0.3                         # dot == 0 is not > 0
    # the two demos' signs: (-zx) * steepen and zx * (-steepen) are the same bits
    rng = np.random.default_rng(2)
    zx, zy = rng.normal(size=1000), rng.normal(size=1000)
    a = M.shade(zx, zy, M.Light(-50.0, 50.0, sun, 0.2))
    nx, ny = -zx * 50.0, zy * 50.0
    s = np.sqrt(nx * nx + ny * ny + 1)
    dot = nx / s * sun[0] + ny / s * sun[1] + 1 / s * sun[2]
    assert np.array_equal(a, np.where(dot > 0, dot * (1 - 0.2) + 0.2, 0.2))


def test_the_packed_table_is_what_the_header_says():
    for name in RC.PALETTES:
        pal = RC.model(name)
        assert len(RC.pack_table(pal)) == 64 + 80 * pal.n
