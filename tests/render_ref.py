"""A numpy model of the reference's colour palette and of its demos' shaded relief, written from the Java and independent of the
C++: imaging/palette/ColorPaletteTable.java (the constructor :162-253, getArgb :395-456, getArgbWithShade :481-541, the
UnlimitedRange forms :567-598), ColorPaletteRecord.java:176-182 (compareTo), ColorPaletteRecordRGB.java:72-121,
ColorPaletteRecordHSV.java:95-194, java.util.Arrays.binarySearch(double[], double) and java.awt.Color.HSBtoRGB as the JDK defines
them, and the illumination model of demo/.../globalDEM/ExtractData.java:405-415 and demo/geoTiff/DemoCOG.java:421-431.

Every arithmetic step is one numpy ufunc, rounded once, in the order in which the Java writes it: float64 for the table and the
records, float32 for HSBtoRGB.  All values of a call are evaluated together.  ARGB words are uint32.

No JVM runs beside these tests: the palette half is pinned by the reference's own assertion (ColorPaletteTableReaderTest.java:56-57)
and by values worked out from its source (tests/test_render_ref.py), the HSBtoRGB half by the JDK's documented definition alone.
"""
import copy

import numpy as np

import interp_ref as R

F8, F4 = np.float64, np.float32
RGB, HSV = 0, 1
CANONICAL_NAN = 0x7ff8000000000000


def double_bits(x):
    """Double.doubleToLongBits: int64, every NaN canonical"""
    x = np.ascontiguousarray(x, F8)
    return np.where(np.isnan(x), np.int64(CANONICAL_NAN), x.view(np.int64))


def java_compare(a, b):
    """Double.compare of two scalars"""
    a, b = F8(a), F8(b)
    if a < b:
        return -1
    if a > b:
        return 1
    x, y = int(double_bits([a])[0]), int(double_bits([b])[0])
    return (x > y) - (x < y)


def java_int_f(x):
    """(int) of a float: a float32 is a double"""
    return R.java_int(np.asarray(x, F4).astype(F8))


def word(r, g, b):
    """0xff000000 | (r << 16) | (g << 8) | b on Java ints"""
    r, g, b = (np.asarray(c, np.int64) & 0xffffffff for c in (r, g, b))
    return ((0xff000000 | (r << 16) | (g << 8) | b) & 0xffffffff).astype(np.uint32)


def binary_search(keys, z):
    """Arrays.binarySearch(double[], double), binarySearch0 as the JDK writes it; int64 per element of z"""
    keys, z = np.asarray(keys, F8), np.asarray(z, F8)
    kb, zb = double_bits(keys), double_bits(z)
    low, high = np.zeros(z.shape, np.int64), np.full(z.shape, len(keys) - 1, np.int64)
    found = np.full(z.shape, -1, np.int64)
    done = np.zeros(z.shape, bool)
    while True:
        active = ~done & (low <= high)
        if not active.any():
            break
        mid = (low + high) >> 1                                          # (>>> 1: both are small and non-negative)
        at = np.where(active, mid, 0)
        mid_val, mid_bits = keys[at], kb[at]
        lt, gt = mid_val < z, mid_val > z
        same = ~lt & ~gt
        hit = active & same & (mid_bits == zb)
        up = lt | (same & (mid_bits < zb))
        found[hit] = mid[hit]
        done |= hit
        low = np.where(active & ~hit & up, mid + 1, low)
        high = np.where(active & ~hit & ~up, mid - 1, high)
    return np.where(done, found, -(low + 1))


def hsb_to_rgb(hue, saturation, brightness):
    """java.awt.Color.HSBtoRGB on float32 arrays"""
    hue, s, v = (np.asarray(x, F4) for x in (hue, saturation, brightness))
    c255, half, one, six = F4(255.0), F4(0.5), F4(1.0), F4(6.0)
    with np.errstate(all="ignore"):
        grey = java_int_f(v * c255 + half)
        h = (hue - np.floor(hue)) * six
        f = h - np.floor(h)
        p = v * (one - s)
        q = v * (one - s * f)
        t = v * (one - (s * (one - f)))
        case = java_int_f(h)
        zero = np.zeros(h.shape, F4)
        pick = lambda table: np.select([case == k for k in range(6)], table, zero)
        fr, fg, fb = pick([v, q, p, p, t, v]), pick([t, v, v, q, p, p]), pick([p, p, t, v, v, q])
        inside = (case >= 0) & (case <= 5)
        r = np.where(inside, java_int_f(fr * c255 + half), 0)
        g = np.where(inside, java_int_f(fg * c255 + half), 0)
        b = np.where(inside, java_int_f(fb * c255 + half), 0)
    achromatic = s == 0
    return word(np.where(achromatic, grey, r), np.where(achromatic, grey, g), np.where(achromatic, grey, b))


class Palette:
    """ColorPaletteTable.  records: tuples (range0, range1, "rgb" | "hsv", c0, c1), c = (r, g, b) integers 0..255 or (h, s, v)
    doubles.  normalized == hinge == False is the first constructor."""

    def __init__(self, records, argb_for_null=0, normalized=False, range_min=0.0, range_max=0.0, hinge=False, hinge_value=0.0):
        assert len(records) >= 1
        recs = list(records)
        # Arrays.sort(Object[]) is stable; compareTo is Double.compare on range0, then range1 (insertion by comparison: n is small)
        order = []
        for r in recs:
            k = len(order)
            while k > 0 and (java_compare(order[k - 1][0], r[0]) or java_compare(order[k - 1][1], r[1])) > 0:
                k -= 1
            order.insert(k, r)
        self.n = len(order)
        self.range0 = np.array([r[0] for r in order], F8)
        self.range1 = np.array([r[1] for r in order], F8)
        self.keys = self.range0.copy()
        self.model = np.array([RGB if r[2] in ("rgb", RGB) else HSV for r in order], np.int32)
        self.c0, self.d = np.zeros((self.n, 3), F8), np.zeros((self.n, 3), F8)
        self.wrap_around = np.zeros(self.n, bool)
        self.source = order
        for i, (_, _, _, c0, c1) in enumerate(order):
            if self.model[i] == RGB:                                     # ColorPaletteRecordRGB.java:76-84
                self.c0[i] = [F8(int(c)) for c in c0]
                self.d[i] = [F8(int(b) - int(a)) for a, b in zip(c0, c1)]
                continue
            h0, s0, v0 = (F8(c) for c in c0)                             # ColorPaletteRecordHSV.java:98-125
            h1, s1, v1 = (F8(c) for c in c1)
            d_h = h1 - h0
            if abs(d_h) < 1.0e-6:
                delta_h = F8(0)
            else:
                if d_h <= -180:
                    d_h = d_h + 360
                elif d_h > 180:
                    d_h = d_h - 360
                if d_h == 0:
                    d_h = F8(360)
                delta_h = d_h
            self.c0[i], self.d[i] = (h0, s0, v0), (delta_h, s1 - s0, v1 - v0)
            self.wrap_around[i] = bool(h0 + delta_h > 360.0 or h0 + delta_h < 0)
        self.argb_for_null = np.uint32(int(argb_for_null) & 0xffffffff)
        self.normalized, self.hinge = bool(normalized), bool(hinge)
        self.norm_min, self.norm_max, self.hinge_value = F8(range_min), F8(range_max), F8(hinge_value)
        self.range_min, self.range_max = self.range0[0], self.range1[-1]              # :234-235
        self.hinge_index = -1
        if self.hinge:
            match = np.flatnonzero(self.range0 == self.hinge_value)
            assert match.size, "Unable to match hinge value"
            self.hinge_index = int(match[0])

    def get_range_min(self):
        return self.norm_min if self.normalized else self.range_min

    def get_range_max(self):
        return self.norm_max if self.normalized else self.range_max

    def _record(self, index, z, shade):
        """records[index].getArgb(z) / getArgbWithShade(z, shade), per element"""
        r0, r1, c0, d = self.range0[index], self.range1[index], self.c0[index], self.d[index]
        t = (z - r0) / (r1 - r0)
        t = np.where(t < 0, F8(0), np.where(t > 1, F8(1), t))
        if shade is None:
            ch = [R.java_int(d[:, k] * t + c0[:, k] + 0.5) for k in range(3)]
        else:
            ch = [R.java_int(shade * (d[:, k] * t + c0[:, k]) + 0.5) for k in range(3)]
        rgb = word(*ch)
        a = d[:, 0] * t + c0[:, 0]
        a = np.where(self.wrap_around[index], np.where(a < 0.0, a + 360.0, np.where(a > 360.0, a - 360.0, a)), a)
        s = (d[:, 1] * t + c0[:, 1]).astype(F4)
        v = (d[:, 2] * t + c0[:, 2]).astype(F4) if shade is None else ((d[:, 2] * t + c0[:, 2]) * shade).astype(F4)
        h = (a / 360.0).astype(F4)
        return np.where(self.model[index] == RGB, rgb, hsb_to_rgb(h, s, v))

    def argb(self, z_target, shade=None, unlimited=False):
        """getArgb (shade None) / getArgbWithShade, with unlimited the UnlimitedRange forms; uint32 per element"""
        z = np.array(z_target, F8).ravel()
        shade = None if shade is None else np.broadcast_to(np.asarray(shade, F8).ravel(), z.shape)
        with np.errstate(all="ignore"):
            if unlimited:                                                # :567-598
                z = np.where(z < self.range_min, self.range_min, np.where(z > self.range_max, self.range_max, z))
            if self.normalized:                                          # :405-420
                last = self.n - 1
                if self.hinge:
                    i0 = self.hinge_index
                    t = (z - self.norm_min) / (self.hinge_value - self.norm_min)
                    below = t * (self.range1[i0 - 1] - self.range0[0]) + self.range0[0]
                    t = (z - self.hinge_value) / (self.norm_max - self.hinge_value)
                    above = t * (self.range1[last] - self.range0[i0]) + self.range0[i0]
                    z = np.where(z < self.hinge_value, below, above)
                else:
                    t = (z - self.norm_min) / (self.norm_max - self.norm_min)
                    z = t * (self.range1[last] - self.range0[0]) + self.range0[0]
            index = binary_search(self.keys, z)
            before = -(index + 1) - 1                                    # :442
            use = np.where(index >= 0, index, np.maximum(before, 0))
            colour = self._record(use, z, shade)
            covered = (index >= 0) | ((index != -1) & (self.range1[use] >= z))
        return np.where(covered, colour, self.argb_for_null).astype(np.uint32)


class Light:
    """the illumination model's constants: the gains on zx and zy (ExtractData: -steepen, +steepen; DemoCOG: both -steepen), the
    vector towards the sun, the ambient level"""

    def __init__(self, x_gain, y_gain, sun, ambient):
        self.x_gain, self.y_gain, self.ambient = F8(x_gain), F8(y_gain), F8(ambient)
        self.sun = tuple(F8(x) for x in sun)


def shade(zx, zy, light):
    """ExtractData.java:405-415"""
    zx, zy = np.asarray(zx, F8), np.asarray(zy, F8)
    with np.errstate(all="ignore"):
        nx = zx * light.x_gain
        ny = zy * light.y_gain
        s = np.sqrt(nx * nx + ny * ny + 1)
        nx = nx / s
        ny = ny / s
        nz = 1 / s
        dot = nx * light.sun[0] + ny * light.sun[1] + nz * light.sun[2]
        lit = dot * (1 - light.ambient) + light.ambient
    return np.where(dot > 0, lit, light.ambient)


def cells_z(cells, elem_type, fill_i=0):
    """the cells of a block as the doubles that are looked up"""
    return R.samples_f32(np.asarray(cells), elem_type, fill_i).astype(F8).ravel()


def render_cells(palette, cells, elem_type, fill_i=0, shades=None, unlimited=False):
    return palette.argb(cells_z(cells, elem_type, fill_i), shades, unlimited)


def render_points(spec, block, rows, cols, palette, light=None, col_spacing=None, unlimited=False):
    """The model of the interpolating render calls: dict argb (uint32), shade (float64, NaN-free; only with a light), status.
    First derivatives are evaluated with a light, the value alone without; spec.target is not looked at."""
    s = copy.copy(spec)
    s.target = R.FIRST if light is not None else R.VALUE
    ip = R.interp(s, block, rows, cols, col_spacing)
    out = {"status": ip["status"]}
    sh = None
    if light is not None:
        sh = out["shade"] = shade(ip["zx"], ip["zy"], light)
    out["argb"] = palette.argb(ip["z"], sh, unlimited)
    return out
