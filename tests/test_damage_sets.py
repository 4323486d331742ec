"""Pins what tests/damage.py produces for a fixed seed and shape (CPU only): the number of damaged packings per kind, that each
kind holds both oracle verdicts, and the oracle's outcome on every crafted M32 stream -- so that the GPU file
test_gpu_damaged_builds.py cannot quietly turn into a set that every decoder rejects."""
import pytest

import damage as D
import oracle
from tilegen import make_tile

R, C = 120, 150
SEED = 1


def _tile(nulls=False):
    v = make_tile("smooth", R, C, seed=1).copy()
    if nulls:
        v[(R * C) // 3:(R * C) // 3 + (R * C) // 5] = oracle.INT4_NULL
    return v


def _outcomes(kind, v, items):
    out = set()
    for _, pk in items:
        out.add("deviation" if D.deviation(pk, kind, R * C) else D.outcome(kind, R, C, pk, v).split()[0])
    return out


@pytest.mark.parametrize("kind,part,count,outcomes", [
    (D.HUFFMAN, "header", 18, {"changed", "deviation", "throws"}),
    (D.HUFFMAN, "tree", 1305, {"changed", "throws"}),
    (D.HUFFMAN, "text", 675, {"changed", "same", "throws"}),
    (D.HUFFMAN, "length", 24, {"same", "throws"}),
    (D.CANON, "header", 20, {"changed", "same", "throws"}),
    (D.CANON, "tree", 591, {"changed", "same", "throws"}),
    (D.CANON, "text", 676, {"changed", "same", "throws"}),
    (D.CANON, "length", 24, {"same", "throws"}),
])
def test_damage_kinds(kind, part, count, outcomes):
    v = _tile()
    enc = oracle.codec_huffman_encode if kind == D.HUFFMAN else oracle.codec_canon_encode
    pk = enc(0, R, C, v)[0]
    items = D.damage_set(pk, kind, R, C, SEED, (part,))
    assert len(items) == count
    assert len({p for _, p in items}) == count and pk not in {p for _, p in items}
    assert _outcomes(kind, v, items) == outcomes


def test_tree_and_table_ends():
    """the tree flips stop 8 bits behind the serialised tree; the canonical ones at the end of the length tables, where the text's
    first flip starts"""
    v = _tile()
    pk = oracle.codec_huffman_encode(0, R, C, v)[0]
    end, deepest = D.huffman_tree_walk(pk)
    assert len(D.tree_damage(pk, D.HUFFMAN)) == end + 8 - 80 and 1 <= deepest <= D.MAX_DEPTH
    cpk = oracle.codec_canon_encode(0, R, C, v)[0]
    tend = D.canon_table_end(cpk)
    assert 48 < tend < len(cpk) * 8 and len(D.tree_damage(cpk, D.CANON)) == tend - 48


def test_deviation_predicates():
    v = _tile()
    pk = oracle.codec_huffman_encode(0, R, C, v)[0]
    assert D.deviation(pk, D.HUFFMAN, R * C) is None
    put = lambda n: pk[:6] + n.to_bytes(4, "little") + pk[10:]
    assert D.deviation(put(6 * R * C), D.HUFFMAN, R * C) is None
    assert D.deviation(put(6 * R * C + 1), D.HUFFMAN, R * C) == "nM32 > 6*cells"
    # a comb of 66 leaves: a leaf and a branch under every branch, the last two leaves at depth 65
    bits = [(65 >> k) & 1 for k in range(8)] + [0]
    for _ in range(64):
        bits += [1] + [0] * 8 + [0]
    bits += [1] + [0] * 8 + [1] + [0] * 8
    raw = bytearray(len(bits) // 8 + 8)
    for i, b in enumerate(bits):
        raw[i >> 3] |= b << (i & 7)
    deep = pk[:10] + bytes(raw)
    assert D.huffman_tree_walk(deep)[1] > D.MAX_DEPTH and D.deviation(deep, D.HUFFMAN, R * C) == "tree deeper than 63"


CRAFTED = {
    "unaltered": "same", "last byte dropped": "throws", "trailing 0x7f": "throws", "trailing 0x81": "throws",
    "0x7f appended": "same", "6-byte value inserted": "changed 17996", "6-byte pair wraps": "changed 17280",
    "extra bytes behind": "same", "3-byte run": "changed 16680", "null code 0x80": "changed 3660",
}
CRAFTED_NULLS = {
    "unaltered": "same", "last byte dropped": "throws", "trailing 0x7f": "throws", "trailing 0x81": "throws",
    "0x7f appended": "same", "6-byte value inserted": "changed 14392", "6-byte pair wraps": "changed 145",
    "extra bytes behind": "same", "3-byte run": "changed 140", "null at row start": "changed 5850", "null after a sum": "changed 149",
}


@pytest.mark.parametrize("kind", [D.HUFFMAN, D.DEFLATE])
@pytest.mark.parametrize("nulls", [False, True])
def test_crafted_m32_outcomes(kind, nulls):
    v = _tile(nulls)
    good, crafted = D.crafted_m32(kind, R, C, v, 5)
    assert crafted[0][1] == good                       # the unaltered stream re-encodes to the oracle's packing byte for byte
    got = {label[len("crafted: "):]: D.outcome(kind, R, C, pk, v) for label, pk in crafted}
    assert got == (CRAFTED_NULLS if nulls else CRAFTED)
    if kind == D.HUFFMAN:
        for label, pk in crafted:                      # a valid packing: the nM32 field is the stream's length
            assert D.huffman_tree_walk(pk)[1] <= D.MAX_DEPTH and D.deviation(pk, kind, R * C) is None, label


def test_seeded():
    v = _tile()
    pk = oracle.codec_huffman_encode(0, R, C, v)[0]
    assert D.damage_set(pk, D.HUFFMAN, R, C, 3) == D.damage_set(pk, D.HUFFMAN, R, C, 3)
    assert D.damage_set(pk, D.HUFFMAN, R, C, 3) != D.damage_set(pk, D.HUFFMAN, R, C, 4)
    assert D.crafted_m32(D.HUFFMAN, R, C, v, 5) == D.crafted_m32(D.HUFFMAN, R, C, v, 5)
