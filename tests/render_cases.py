"""Inputs shared by the render tests (tests/test_render_ref.py, tests/test_render_shared_header.py and tests/test_render_args.py on
the CPU, tests/test_gpu_render.py on the GPU): the reference's palette files read as data, a catalogue of palettes that takes every
branch of the lookup, the z values at which a lookup can go wrong, and the glue between the model's Palette (tests/render_ref.py),
the packed table of gridfour_amd/csrc/gvrs_render_common.h, the stand-alone CPU harness and the library's gf_palette_spec."""
import os
import struct
import subprocess

import numpy as np

import interp_cases as K
import interp_ref as R
import render_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
PALETTE_DIR = os.path.join(HERE, "golden", "palettes")

# GfPalHead and GfPalRec (gridfour_amd/csrc/gvrs_render_common.h)
HEAD = np.dtype([("n", np.int32), ("argb_for_null", np.uint32), ("normalized", np.int32), ("hinge", np.int32), ("hinge_index", np.int32),
                 ("pad", np.int32), ("range_min", np.float64), ("range_max", np.float64), ("norm_min", np.float64), ("norm_max", np.float64),
                 ("hinge_value", np.float64)])
REC = np.dtype([("range0", np.float64), ("range1", np.float64), ("c0", np.float64, 3), ("d", np.float64, 3), ("model", np.int32),
                ("wrap_around", np.int32)])
assert HEAD.itemsize == 64 and REC.itemsize == 72


def read_cpt(name):
    """(records, argb_for_null) of a palette file of the reference: the two record spellings its three test files use,
    `z r g b z r g b` and `z r/g/b z r/g/b ;label`; F, B and # lines are skipped, N's colour is the null colour"""
    records, null = [], 0
    for line in open(os.path.join(PALETTE_DIR, name)):
        line = line.split(";")[0].replace("/", " ").strip()
        if not line or line[0] in "#FB":
            continue
        tok = line.split()
        if tok[0] == "N":
            r, g, b = (int(t) for t in tok[1:4])
            null = 0xff000000 | r << 16 | g << 8 | b
            continue
        v = [float(t) for t in tok[:8]]
        records.append((v[0], v[4], "rgb", tuple(int(c) for c in v[1:4]), tuple(int(c) for c in v[5:8])))
    return records, null


def cpt(name, **kw):
    records, null = read_cpt(name)
    return dict(records=records, argb_for_null=null, **kw)


def _ramp(n, lo=-100.0, hi=100.0, gaps=False):
    """n RGB records that tile lo .. hi; with gaps every third one ends early"""
    edges = np.linspace(lo, hi, n + 1)
    recs = []
    for i in range(n):
        top = edges[i + 1] if not (gaps and i % 3 == 1) else edges[i] + (edges[i + 1] - edges[i]) * 0.4
        recs.append((float(edges[i]), float(top), "rgb", ((37 * i) % 256, (91 * i + 5) % 256, (13 * i + 200) % 256),
                     ((53 * i + 9) % 256, (7 * i + 77) % 256, (201 * i) % 256)))
    return recs


HSV_RECORDS = [(-50.0, 0.0, "hsv", (350.0, 0.9, 0.4), (10.0, 0.5, 1.0)),         # wraps upward through 360
               (0.0, 10.0, "hsv", (10.0, 0.5, 1.0), (350.0, 1.0, 0.25)),         # wraps downward through 0
               (10.0, 20.0, "hsv", (360.0, 1.0, 1.0), (360.0, 0.0, 1.0)),        # hue exactly 360; saturation reaches 0
               (20.0, 30.0, "hsv", (-1e-7, 1.0, 1.0), (10.0, 1.0, 1.0)),         # a hue just below 0 without wrap-around: 6.0f, black
               (30.0, 40.0, "hsv", (0.0, 0.75, 0.5), (180.0, 0.25, 0.75)),       # a span of 180
               (40.0, 50.0, "hsv", (200.0, 0.0, 0.3), (200.0, 0.0, 0.9)),        # saturation 0 throughout
               (50.0, 60.0, "hsv", (90.0, 0.3, 0.2), (270.0 - 1e-9, 0.8, 0.6)),
               (60.0, 70.0, "rgb", (1, 2, 3), (250, 128, 0))]                    # both models in one table

# name -> the arguments of render_ref.Palette (and of gridfour_amd.Palette)
PALETTES = {
    "etopo1": lambda: cpt("ETOPO1.cpt"),
    "ocean": lambda: cpt("OceanBasemap.cpt"),
    "categorical": lambda: cpt("CategoricalPaletteWithNames.cpt"),
    "one": lambda: dict(records=[(-3.5, 7.25, "rgb", (10, 20, 30), (200, 100, 0))], argb_for_null=0x01020304),
    "two_equal_keys": lambda: dict(records=[(5.0, 9.0, "rgb", (0, 0, 255), (255, 0, 0)), (5.0, 6.0, "rgb", (0, 255, 0), (9, 9, 9))],
                                   argb_for_null=0xff808080),
    "point_records": lambda: dict(records=[(1.0, 1.0, "rgb", (9, 8, 7), (6, 5, 4)), (2.0, 2.0, "rgb", (90, 80, 70), (60, 50, 40)),
                                           (-0.0, 0.5, "rgb", (1, 1, 1), (2, 2, 2)), (0.0, 0.25, "rgb", (3, 3, 3), (4, 4, 4))],
                                  argb_for_null=0),
    "gaps_256": lambda: dict(records=_ramp(256, -1000.0, 1000.0, gaps=True), argb_for_null=0xff112233),
    "normalized": lambda: dict(records=_ramp(7, 0.0, 1.0), argb_for_null=0xffabcdef, normalized=True, range_min=-250.0, range_max=4000.0),
    "hinge": lambda: dict(records=_ramp(8, -1.0, 1.0), argb_for_null=0xff010101, normalized=True, range_min=-8000.0, range_max=2500.0,
                          hinge=True, hinge_value=0.0),
    "hsv": lambda: dict(records=HSV_RECORDS, argb_for_null=0x80ff00ff),
}


def model(name):
    return M.Palette(**PALETTES[name]())


def lookup_z(pal, rng, n_random=1000):
    """the z values of a lookup test, in the palette's INPUT range: random ones over the range and a margin, every key and every
    range1 with both neighbours (nextafter), and the special values"""
    lo, hi = float(pal.get_range_min()), float(pal.get_range_max())
    span = hi - lo if hi > lo else 1.0
    edges = np.concatenate([pal.range0, pal.range1])
    if pal.normalized:                                                   # back into the input range (roughly: the neighbours are added below)
        edges = lo + (edges - pal.range_min) / (pal.range_max - pal.range_min) * span
        if pal.hinge:
            edges = np.concatenate([edges, [float(pal.hinge_value)]])
    near = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)])
    special = [0.0, -0.0, np.nan, np.inf, -np.inf, lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), lo - 0.5, hi + 1e-7,
               1e300, -1e300, 5e-324, -5e-324, 2.0 ** 31, -2.0 ** 31]
    return np.concatenate([rng.uniform(lo - 0.1 * span, hi + 0.1 * span, n_random), near, special])


def shades_for(rng, n):
    """a shade per value: most in 0..1, some exact ends, some outside, some NaN"""
    s = rng.uniform(0.0, 1.0, n)
    s[::7], s[1::11], s[2::13], s[3::17], s[4::19] = 1.0, 0.0, 1.5, np.nan, -0.25
    return s


def pack_table(pal):
    """the model's Palette as the packed table GfPalHead | keys[n] | recs[n]"""
    h = np.zeros(1, HEAD)
    h["n"], h["argb_for_null"], h["normalized"], h["hinge"], h["hinge_index"] = pal.n, pal.argb_for_null, pal.normalized, pal.hinge, pal.hinge_index
    h["range_min"], h["range_max"], h["norm_min"], h["norm_max"], h["hinge_value"] = pal.range_min, pal.range_max, pal.norm_min, pal.norm_max, pal.hinge_value
    r = np.zeros(pal.n, REC)
    r["range0"], r["range1"], r["c0"], r["d"], r["model"], r["wrap_around"] = pal.range0, pal.range1, pal.c0, pal.d, pal.model, pal.wrap_around
    return h.tobytes() + pal.keys.astype(np.float64).tobytes() + r.tobytes()


# ---------------------------------------------------------------- the stand-alone CPU harness (tests/csrc/render_harness.cpp)

def build_harness(flags=("-O2", "-ffp-contract=off"), name="render_harness"):
    src, exe = os.path.join(HERE, "csrc", "render_harness.cpp"), os.path.join(HERE, "csrc", name)
    subprocess.check_call(["g++", *flags, "-std=c++17", "-o", exe, src])
    return exe


def _run(exe, mode, payload, tmp):
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(payload)
    subprocess.run([exe, mode, src, dst], check=True)
    return open(dst, "rb").read()


def _blob(b):
    return struct.pack("<q", len(b)) + b


def harness_lookup(exe, tmp, pal, values, shades=None, unlimited=False, elem_type=-1, fill_i=0):
    """values: doubles (elem_type -1) or the cells of a block -> uint32 words; pal: the model's Palette, or a packed table's bytes"""
    values = np.ascontiguousarray(values)
    payload = _blob(pal if isinstance(pal, bytes) else pack_table(pal)) + struct.pack("<qiiii", values.size, elem_type, fill_i, shades is not None, unlimited) + _blob(values.tobytes())
    if shades is not None:
        payload += np.ascontiguousarray(shades, np.float64).tobytes()
    return np.frombuffer(_run(exe, "lookup", payload, tmp), np.uint32)


def harness_lattice(exe, tmp, spec, block, lattice, pal, light=None, cs_rows=None, unlimited=False):
    """the model's render_points on a lattice -> dict argb, shade, status"""
    s = R.Spec.__new__(R.Spec)
    s.__dict__.update(spec.__dict__)
    s.target = R.FIRST if light is not None else R.VALUE
    n = lattice[4] * lattice[5]
    payload = _blob(pack_table(pal)) + _blob(K.geom_of(s).tobytes()) + _blob(np.ascontiguousarray(block).tobytes())
    payload += struct.pack("<ddddqq", *lattice) + struct.pack("<iii", cs_rows is not None, light is not None, unlimited)
    if cs_rows is not None:
        payload += np.ascontiguousarray(cs_rows, np.float64).tobytes()
    if light is not None:
        payload += struct.pack("<dddddd", light.x_gain, light.y_gain, *light.sun, light.ambient)
    raw = _run(exe, "lattice", payload, tmp)
    return {"argb": np.frombuffer(raw, np.uint32, n), "shade": np.frombuffer(raw, np.float64, n, 4 * n + (4 * n) % 8),
            "status": np.frombuffer(raw, np.int32, n, 4 * n + (4 * n) % 8 + 8 * n)}


# ---------------------------------------------------------------- the library

def lib_palette_args(name):
    """the arguments of gridfour_amd.Palette / palette_spec for a catalogue entry"""
    return PALETTES[name]()


def lib_light(light):
    import gridfour_amd
    return None if light is None else gridfour_amd.render_light(light.x_gain, light.y_gain, light.sun, light.ambient)


LIGHTS = {"extract": M.Light(-50.0, 50.0, (-0.40957602214449595, 0.28678821817552297, 0.8660254037844386), 0.2),      # ExtractData: 145 / 60 degrees
          "cog": M.Light(-3.5, -3.5, (0.3535533905932738, -0.6123724356957945, 0.7071067811865476), 0.25)}              # DemoCOG's signs


def same_shade(a, b):
    return R.same_bits(a, b)
