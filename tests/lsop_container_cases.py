"""The LSOP12 / LSOP08 batches whose container choice is pinned, shared by test_lsop_container_header.py (CPU) and
test_gpu_lsop_host_forms.py: per tile what the device encoder leaves for the host (status, its packing, the 16-word coefficient
record, the residual streams) and what the host form must answer (packing, container type), all from the references
(oracle.lsop12_*, lsop08_ref).  Computed once per process and left unchanged."""
import functools
import struct

import numpy as np

import lsop08_ref as R
import oracle
from tilegen import make_tile

OK, DECLINED = 0, 1
CODEC_INDEX = 2

# name -> (family, rows, columns, tile kinds, Deflate enabled, value checksum); the declined tile (uniform) lies between two good ones
BATCHES = {
    "lsop12_48": (12, 48, 48, ("smooth", "uniform", "ramp"), True, False),
    "lsop12_48_checksum": (12, 48, 48, ("smooth", "uniform", "ramp"), True, True),
    "lsop12_48_no_deflate": (12, 48, 48, ("smooth", "uniform", "ramp"), False, False),
    "lsop12_6": (12, 6, 6, ("terrain",), True, False),
    "lsop08_6": (8, 6, 6, ("terrain",), True, False),
    "lsop08_7x9": (8, 7, 9, ("terrain", "uniform", "smooth"), True, False),
    "lsop08_4": (8, 4, 4, ("terrain",), True, False),
}


class Tile:
    """status: the device encoder's; device: its packing (b"" when declined); coefs: uint32[16]; residuals: int32, initialisers then
    interior; want, want_type: the host form's packing (None when declined) and container type"""

    def __init__(self, status, device, coefs, residuals, want, want_type):
        self.status, self.device, self.coefs, self.residuals, self.want, self.want_type = status, device, coefs, residuals, want, want_type


class Batch:
    def __init__(self, name):
        self.name = name
        self.family, self.nr, self.nc, self.kinds, self.deflate, self.checksum = BATCHES[name]
        self.values = np.stack([R.terrain(self.nr, self.nc, 0) if k == "terrain" else make_tile(k, self.nr, self.nc) for k in self.kinds])
        self.tiles = [(_tile12 if self.family == 12 else _tile08)(self, v) for v in self.values]
        self.flags = (1 if self.deflate else 0) | (2 if self.checksum else 0)

    @property
    def n_res(self):
        nr, nc = self.nr, self.nc
        return 4 * nr + 2 * nc - 9 + (nr - 2) * (nc - 4) if self.family == 12 else 2 * nr + 2 * nc - 5 + (nr - 2) * (nc - 2)

    def want_blob(self):
        """(blob, offsets, types, statuses) of the host form"""
        packs = [t.want or b"" for t in self.tiles]
        return (b"".join(packs), np.cumsum([0] + [len(p) for p in packs]).tolist(), [t.want_type for t in self.tiles],
                [t.status for t in self.tiles])


def _declined(b):
    return Tile(DECLINED, b"", np.zeros(16, np.uint32), np.zeros(b.n_res, np.int32), None, 0)


def _tile12(b, v):
    pr = oracle.lsop12_residuals(b.nr, b.nc, v)
    want, want_type = oracle.lsop12_encode(CODEC_INDEX, b.nr, b.nc, v, b.deflate, b.checksum)
    if pr is None:
        assert want is None
        return _declined(b)
    seed, u, init, inter = pr
    device, t = oracle.lsop12_encode(CODEC_INDEX, b.nr, b.nc, v, False, b.checksum)
    assert t == 2
    coefs = np.zeros(16, np.uint32)
    coefs[0] = seed & 0xFFFFFFFF
    coefs[1:13] = u.view(np.uint32)
    if b.checksum:
        coefs[13], = struct.unpack_from("<I", device, 55)          # LsHeader.packHeader: behind the coefficients
    return Tile(OK, device, coefs, np.concatenate([init, inter]).astype(np.int32), want, want_type)


def _tile08(b, v):
    pr = R.predict(b.nr, b.nc, v)
    if pr is None:
        return _declined(b)
    seed, u, init, inter = pr
    device = R.encode(CODEC_INDEX, b.nr, b.nc, v, force_type=0)[0]
    want, want_type = R.encode(CODEC_INDEX, b.nr, b.nc, v)
    coefs = np.zeros(16, np.uint32)
    coefs[0] = seed & 0xFFFFFFFF
    coefs[1:9] = u.view(np.uint32)
    return Tile(OK, device, coefs, np.array(init + inter, np.int64).astype(np.int32), want, want_type)


@functools.lru_cache(maxsize=None)
def batch(name):
    return Batch(name)
