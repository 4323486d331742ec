"""Decoder robustness on damaged packings, held to the oracle's verdict: where the oracle decodes the damaged packing, the
device returns status 0 and the oracle's values; where the oracle throws, the device returns GF_ERR_FORMAT or GF_ERR_BOUNDS
(the reference's exception there is of some kind; which one is not part of the contract).  The documented deviations of
DESIGN.md 2 (damage.deviation) must give one of those errors whatever the oracle does."""
import numpy as np
import pytest

import damage
import oracle
from tilegen import add_nulls, make_tile

pytestmark = pytest.mark.gpu

ERRORS = {-1, -2}                  # FORMAT, BOUNDS


def _damage(rng, packing, n_variants):
    out = []
    p = bytearray(packing)
    for i in range(n_variants):
        q = bytearray(p)
        kind = i % 5
        if kind == 0:                                   # single bit flip anywhere
            j = int(rng.integers(0, len(q) * 8))
            q[j >> 3] ^= 1 << (j & 7)
        elif kind == 1:                                 # bit flips in the code-table region
            for _ in range(3):
                j = int(rng.integers(16, min(len(q), 200) * 8))
                q[j >> 3] ^= 1 << (j & 7)
        elif kind == 2:                                 # truncation
            q = q[:int(rng.integers(1, len(q)))]
        elif kind == 3:                                 # random bytes in the middle
            a = int(rng.integers(10, max(11, len(q) - 8)))
            q[a:a + 8] = bytes(rng.integers(0, 256, 8, dtype=np.uint8))
        else:                                           # header damage
            j = int(rng.integers(0, min(10, len(q))))
            q[j] = int(rng.integers(0, 256))
        out.append(bytes(q))
    return out


def _tiles(n_rows, n_cols):
    return [make_tile("smooth", n_rows, n_cols), make_tile("noise16", n_rows, n_cols),
            add_nulls(make_tile("smooth", n_rows, n_cols), n_rows, n_cols, 0.1), make_tile("sparse_big", n_rows, n_cols)]


@pytest.mark.parametrize("family", ["huffman", "canon", "lsop"])
def test_damaged_packings(family):
    import gridfour_amd
    n_rows, n_cols = 40, 60
    rng = np.random.default_rng({"huffman": 1, "canon": 2, "lsop": 3}[family])
    if family == "huffman":
        codec, enc, dec = gridfour_amd.CodecHuffmanHip(), oracle.codec_huffman_encode, oracle.codec_huffman_decode
    elif family == "canon":
        codec, enc, dec = gridfour_amd.CodecCanonHuffmanHip(), oracle.codec_canon_encode, oracle.codec_canon_decode
    else:
        codec = gridfour_amd.LsCodecHip(deflate_enabled=False)
        enc = lambda ci, r, c, v: oracle.lsop12_encode(ci, r, c, v, False)
        dec = oracle.lsop12_decode
    damaged = []
    for v in _tiles(n_rows, n_cols):
        ref = enc(1, n_rows, n_cols, v)[0]
        if ref is None:
            continue
        damaged += _damage(rng, ref, 60)
    vals, status = codec.decode_batch(n_rows, n_cols, damaged)
    n_ok = n_err = 0
    wrong = []
    kind = {"huffman": damage.HUFFMAN, "canon": damage.CANON}.get(family)
    for i, pk in enumerate(damaged):
        st = int(status[i])
        if kind is not None and damage.deviation(pk, kind, n_rows * n_cols) is not None:
            if st not in ERRORS:
                wrong.append((i, st, "deviation"))
            continue
        try:
            want = dec(n_rows, n_cols, pk)
        except (IOError, ValueError):
            want = None
        if want is None:
            n_err += 1
            if st not in ERRORS:
                wrong.append((i, st, "oracle throws"))
        else:
            n_ok += 1
            if st != 0 or not np.array_equal(vals[i], want):
                wrong.append((i, st, "oracle decodes"))
    assert not wrong, (len(wrong), wrong[:12])
    assert n_ok > 0 and n_err > 0   # some damage is harmless (padding bits, unused table entries), some is fatal
