"""The inputs of the record-write tests (gf_tile_record_encode_batch_elems[_dev]) and what the reference would write for them,
computed with the oracle alone: per element and listed codec oracle.codec_huffman_encode / oracle.codec_canon_encode, the
CodecMaster rule (the strictly shortest non-null packing, list order on ties), the per-element rule (not shorter than the standard
size -> the standard form) and the Python framer of tests/test_gpu_records_dev.py.  Nothing here touches a GPU:
tests/test_records_encode_inputs.py holds the batches to the conditions the GPU tests rely on, on the CPU."""
import functools

import numpy as np

from tilegen import KINDS, add_nulls, make_tile

NULL = -2**31
NAN = np.float32(np.nan)
HUFFMAN, DEFLATE, NONE, CANON, LSOP = 1, 2, 0, 3, 4
ICF3 = ("icf", 100.0, -5.25, -9999, NAN)
ELEMS3 = ["short", ICF3, "float"]
ELEMS16 = ["int"] * 16
ELEMENT_SETS = {"int": ["int"], "short": ["short"], "three": ELEMS3, "sixteen": ELEMS16}
SHAPES = [(16, 20), (40, 60), (7, 9)]
LISTS = [(HUFFMAN,), (CANON,), (HUFFMAN, CANON), (CANON, HUFFMAN), (HUFFMAN, NONE, CANON)]
SHORT_FILL = -32768


def kind_of(el):
    return el if isinstance(el, str) else el[0]


def std_size(el, cells):
    """TileElement.java:86-93: bytes per sample * cells, rounded up to a multiple of 4"""
    return (2 * cells + 3) & ~3 if kind_of(el) == "short" else 4 * cells


def _draw(e, i, nr, nc):
    """tile i of element e as int32 cells: a tilegen kind from a fixed sequence; every 11th tile all null, every 7th with a block of
    nulls.  Element e's sequence is shifted against element 0's so that a record mixes kinds."""
    k = (5 * i + 3 * e + i // len(KINDS)) % len(KINDS)
    if (i + 4 * e) % 11 == 10:
        return np.full(nr * nc, NULL, np.int32)
    t = make_tile(KINDS[k], nr, nc, seed=1000 * e + i).astype(np.int32)
    if (i + e) % 7 == 3:
        t = add_nulls(t, nr, nc, 0.3, seed=i, blocks=True)
    return t


def element_values(el, e, nr, nc, nt):
    """[nt, cells] in the type the calls take: int32 (int; icf: the codes), int16 (short; null -> the fill value), float32"""
    tiles = np.stack([_draw(e, i, nr, nc) for i in range(nt)])
    kind = kind_of(el)
    if kind == "short":
        return np.where(tiles == NULL, SHORT_FILL, np.clip(tiles, -32767, 32767)).astype(np.int16)
    if kind == "float":
        with np.errstate(all="ignore"):
            f = (np.where(tiles == NULL, 0, tiles).astype(np.float64) / 7.0).astype(np.float32)
        f[tiles == NULL] = NAN
        b = f.view(np.uint32).copy()
        b[:, 1::97] = 0x80000000                                    # -0.0
        b[:, 5::89] = 0x7fc12345                                    # NaNs with payloads
        b[:, 7::83] = 0xffa00001
        return b.view(np.float32)
    return tiles


def codec_cells(el, values):
    """what TileElement*.encode hands to CodecMaster: int32 cells (short: fill -> INT4_NULL_CODE), None for a float element"""
    kind = kind_of(el)
    if kind == "float":
        return None
    if kind == "short":
        return np.where(values == SHORT_FILL, NULL, values.astype(np.int32)).astype(np.int32)
    return values.astype(np.int32)


def standard_form(el, values_row):
    kind = kind_of(el)
    if kind == "short":
        b = values_row.astype("<i2").tobytes()
        return b + b"\0" * (-len(b) % 4)
    if kind == "float":
        return np.ascontiguousarray(values_row, np.float32).view("<u4").tobytes()
    return values_row.astype("<i4").tobytes()


def _oracle_pack(codec, k, nr, nc, cells_row):
    import oracle
    enc = oracle.codec_huffman_encode if codec == HUFFMAN else oracle.codec_canon_encode
    pk = enc(k, nr, nc, cells_row)
    return pk[0] if isinstance(pk, tuple) else pk


class Batch:
    """nt tiles of len(elems) elements: values[e] is what the calls take, indices the tile indices"""

    def __init__(self, elems, nr, nc, nt):
        self.elems, self.nr, self.nc, self.nt = list(elems), nr, nc, nt
        self.values = [element_values(el, e, nr, nc, nt) for e, el in enumerate(self.elems)]
        self.indices = (np.arange(nt, dtype=np.int64) * 7 + 1000).astype(np.int32)
        self._cand = {}

    def head(self, nt):
        """the first nt tiles as a batch of their own (sharing the oracle's packings)"""
        b = Batch.__new__(Batch)
        b.elems, b.nr, b.nc, b.nt = self.elems, self.nr, self.nc, nt
        b.values = [v[:nt] for v in self.values]
        b.indices = self.indices[:nt]
        b._cand = self._cand
        return b

    def candidate(self, e, t, codec, k):
        key = (e, t, codec, k)
        if key not in self._cand:
            self._cand[key] = _oracle_pack(codec, k, self.nr, self.nc, codec_cells(self.elems[e], self.values[e][t]))
        return self._cand[key]

    def plan(self, codecs):
        """per element and tile (element bytes, winning list index or 255, why: 'packed' | 'not shorter' | 'declined' | 'no codec',
        tie: the winner's length was matched by a later codec of the list)"""
        out = []
        cells = self.nr * self.nc
        for e, el in enumerate(self.elems):
            row = []
            for t in range(self.nt):
                best, best_k, tie, any_pack = None, 255, False, False
                if kind_of(el) != "float":
                    for k, codec in enumerate(codecs):
                        if codec not in (HUFFMAN, CANON):
                            continue
                        pk = self.candidate(e, t, codec, k)
                        if pk is None:
                            continue
                        any_pack = True
                        if best is None or len(pk) < len(best):
                            best, best_k, tie = pk, k, False
                        elif len(pk) == len(best):
                            tie = True
                has_codec = kind_of(el) != "float" and any(c in (HUFFMAN, CANON) for c in codecs)
                if best is not None and len(best) < std_size(el, cells):
                    row.append((best, best_k, "packed", tie))
                else:
                    why = "not shorter" if any_pack else "declined" if has_codec else "no codec"
                    row.append((standard_form(el, self.values[e][t]), 255, why, False))
            out.append(row)
        return out

    def expected(self, codecs, crc=True):
        """(records: list[bytes], codec_used [n_elems, nt]) as the reference would write them"""
        from test_gpu_records_dev import _frame_elems
        plan = self.plan(codecs)
        records = [_frame_elems(int(self.indices[t]), [plan[e][t][0] for e in range(len(self.elems))], crc=crc) for t in range(self.nt)]
        used = np.array([[plan[e][t][1] for t in range(self.nt)] for e in range(len(self.elems))], np.uint8)
        return records, used


@functools.lru_cache(maxsize=None)
def pool(set_name, nr, nc):
    """the tiles every GPU test of one element set and shape draws from: 1,025 at 16 x 20 (the scan's second block of 1,024; 65 for the
    sixteen-element set), 65 otherwise"""
    nt = 1025 if (nr, nc) == (16, 20) and set_name != "sixteen" else 65
    return Batch(ELEMENT_SETS[set_name], nr, nc, nt)


def gpu_batches():
    """(set name, shape, n_tiles) of every batch the byte-for-byte GPU test runs"""
    out = []
    for name in ELEMENT_SETS:
        for shape in SHAPES:
            for nt in (1, 63, 64, 65):
                out.append((name, shape, nt))
        if name != "sixteen":
            out.append((name, (16, 20), 1025))
    return out
