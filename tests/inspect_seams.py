"""Test-only, CPU-only: file images that cross the count and segment seams of gf_file_inspect_dev (gvrs_file_inspect.hip), which the
images of tests/inspect_cases.py (48 tiles, a few KB, 5 to 10 segments) stay far below.  Built from the same parts -- build_image
and standard_record of tests/gvrs_file_build.py, 16-byte metadata records, free nodes whose CRC covers the 8 head bytes, the
library's host gf_crc32c -- on a grid of 64 x 80 tiles of 4 x 4 INT cells.

Every builder returns (image, ledger).  The LEDGER is the file-order list (pos, size, type, tile_index, damaged) of the records as
the walk meets them, kept while the bytes were laid; damaged is "" (sound), "crc" (the checksum fails) or "type9" (the type byte
is 9: a structural stop).  expect(ledger) derives the report from it by the inspector's rules and without the library;
tests/test_inspect_seams_inputs.py holds gf_file_inspect to it and proves, from the ledger and gf_file_inspect_plan, that every
image crosses the seam it is named for (model() restates the anchors and the chain of walks for that).

  many_tiles      5,120 shuffled tile records behind 3 metadata records: 20 workgroups of directory entries, > 256 segments,
                  > 1,024 records in k_inspect_fold
  many_records    40 tile records among 16-byte metadata records, the count on each side of k_inspect_crc's 32,768 waves
  long_span       > 2,048 segments around a free node of 1.5 MiB; links that do not close behind segment 1,024
  large_records   four records of more than one wave's chunks, up to 2 x 1,024 chunks and a part
  many_large      1,030 records k_inspect_crc hands on
  wide_segments   about 40 MB: a segment size above the smallest and no power of two
The segment and chunk sizes come from GvrsFileHip.inspect_plan; the launch constants are literals here only."""
import struct

import numpy as np

import gvrs_file_build as B
import inspect_cases as K
from gridfour_amd import GvrsFileHip

GRID = (256, 320, 4, 4)                    # 64 x 80 tiles of 4 x 4 cells
N_TILE_ROWS, N_TILE_COLS, N_TILES = 64, 80, 5120
ELEMENTS = K.ELEMENTS
TILE_BYTES = 88                            # a standard-form record of 16 INT cells

ANCHOR_GROUP = 256                         # k_inspect_anchors: `blockIdx.x * 256u + threadIdx.x` (gvrs_file_inspect.hip:58)
SEGMENT_GROUP = 256                        # k_inspect_walk, k_inspect_list: the same (gvrs_file_inspect.hip:78, :187)
CHAIN_ROUND = 1024                         # INS_THREADS: a round of k_inspect_chain's scan and of k_inspect_fold (gvrs_file_inspect.hip:42)
CRC_WAVES = 8192 * 4                       # k_inspect_crc: at most 8192 workgroups (gvrs_file_inspect.hip:401) of 4 waves (:248)
LARGE_WAVES = 256 * 4                      # k_inspect_crc_large: 256 workgroups of 256 threads (gvrs_file_inspect.hip:413, :273)
MAX_SEGMENTS = 32768                       # GF_INSPECT_MAX_SEGMENTS (gvrs_file_inspect.h:26)
MIN_SEGMENT = 1024                         # GF_INSPECT_MIN_SEGMENT (gvrs_file_inspect.h:25)
WAVE_CHUNKS = K.WAVE_CHUNKS                # GF_INSPECT_WAVE_CHUNKS (gvrs_file_inspect.h:28)

END, BAD_TILE_INDEX, TILE_TOO_LARGE, TWO_CHECKSUM_FAILURES, BAD_RECORD_TYPE, BAD_RECORD_SIZE, TRUNCATED = range(7)   # gf_inspect_stop


def content_pos(checksums=True):
    return len(B.header_record(GRID, ELEMENTS, (), checksums))


_TILES = {}


def tile_record(tile, checksums=True):
    key = (tile, checksums)
    if key not in _TILES:
        _TILES[key] = K.tile_record(tile, checksums)
        assert len(_TILES[key]) == TILE_BYTES
    return _TILES[key]


class Layout:
    """The content of an image laid record by record, and the ledger of what the walk meets in it"""

    def __init__(self, checksums=True):
        self.checksums = checksums
        self.content = content_pos(checksums)
        self.at = self.content
        self.items = []                    # (bytes, the tile the directory names by them | None)
        self.ledger = []
        self.overrides = {}                # tile -> the position its entry names instead

    def segment(self, seg=MIN_SEGMENT):
        return (self.at - self.content) // seg

    def _lay(self, rec, rtype, tile=-1, named=False, damaged="", size=None):
        self.items.append((rec, tile if named else None))
        self.ledger.append((self.at, len(rec) if size is None else size, rtype, tile, damaged))
        self.at += len(rec)

    def tile(self, tile, named=True):
        self._lay(tile_record(tile, self.checksums), 2, tile, named)

    def meta(self, size, seed):
        self._lay(K.other(1, size, seed, self.checksums), 1)

    def meta16(self, n, seed):
        """n metadata records of 16 bytes, the smallest record there is: [16][type 1][4 bytes][CRC-32C]"""
        body = np.random.default_rng(seed).integers(0, 256, (n, 4), dtype=np.uint8)
        head = struct.pack("<i", 16) + bytes([1, 0, 0, 0])
        for k in range(n):
            rec = head + body[k].tobytes()
            self._lay(rec + struct.pack("<I", B.crc32c(rec) if self.checksums else 0), 1)

    def free(self, size, garbage=False):
        self._lay(K.free_node(size, self.checksums, garbage), 0)

    def to_seam(self, seg=MIN_SEGMENT, multiple=1, seed=99):
        """a metadata record that ends exactly on the next seam whose segment number is a multiple of `multiple`"""
        step = seg * multiple
        size = step - (self.at - self.content) % step
        self.meta(size if size >= 16 else size + step, seed)
        assert (self.at - self.content) % step == 0

    def size_word_too_large(self, tile):
        """Behind a seam: a metadata record of 64 bytes whose size word says 80, then the record the directory names for `tile`, whose
        cells, 16 bytes in, are the head of a metadata record that ends with it (its checksum word is that record's).  The walk
        steps over the tile record's start -- an anchor, the first of its segment -- and goes on from the record inside."""
        self.to_seam()
        rec = bytearray(K.other(1, 64, 7, self.checksums))
        struct.pack_into("<i", rec, 0, 80)
        self._lay(bytes(rec), 1, damaged="crc", size=80)
        cells = (np.arange(16, dtype=np.int32) * 3 + tile * 7).reshape(4, 4)
        cells[0, 0], cells[0, 1] = TILE_BYTES - 16, 1
        host = bytearray(B.standard_record(tile, [cells], self.checksums))
        if self.checksums:
            struct.pack_into("<I", host, TILE_BYTES - 4, B.crc32c(host[16:TILE_BYTES - 4]))
        self.items.append((bytes(host), tile))
        self.ledger.append((self.at + 16, TILE_BYTES - 16, 1, -1, ""))
        self.at += TILE_BYTES

    def false_anchor(self, tile):
        """Behind a seam: a metadata record of 200 bytes that holds, 16 bytes in, what looks like the head of a record of `tile`, and
        the tile's directory entry names that place: an anchor, the first of its segment, the walk never lands on"""
        self.to_seam()
        rec = bytearray(B.other_record(1, 200 - 8, tile))
        struct.pack_into("<iii", rec, 16, TILE_BYTES, 2, tile)
        self.overrides[tile] = self.at + 16 + 8
        self._lay(K.with_crc(bytes(rec), self.checksums), 1)

    def build(self, extended=False, dir_rect=None):
        records, order, gaps, pending = {}, [], {}, []
        for rec, named in self.items:
            if named is None:
                pending.append(rec)
                continue
            assert named not in records, "two records the directory names for one tile"
            records[named] = rec
            gaps[len(order)] = b"".join(pending)
            order.append(named)
            pending = []
        assert not pending, "a layout ends with a named tile record (the directory follows)"
        raw = {t: (p if extended else p // 8) for t, p in self.overrides.items()}
        image, _ = B.build_image(GRID, ELEMENTS, records, (), self.checksums, order=order, between=lambda k: gaps[k], dir_rect=dir_rect,
                                 extended=extended, entry_overrides=raw or None)
        return image, self.ledger + [(self.at, len(image) - self.at, 5, -1, "")]


# ---- damage ----------------------------------------------------------------------------------------------------------------------

def damaged(image, ledger, crc=(), type9=(), at=None):
    """(image, ledger) with the records of these numbers damaged: crc -- one bit of the payload flipped (at: {number: offset in the
    record} for another byte than the first of the payload); type9 -- the type byte set to 9"""
    b, ledger = bytearray(image), list(ledger)
    for k in crc:
        pos, size, rtype, tile, was = ledger[k]
        assert was == "" and rtype != 0 and size >= 16
        off = (at or {}).get(k, 16 if rtype == 2 else 8)           # (a tile record's first cell, another record's content)
        assert 8 <= off < size - 4 and not (rtype == 2 and off < 12)
        b[pos + off] ^= 0x40
        ledger[k] = (pos, size, rtype, tile, "crc")
    for k in type9:
        pos, size, rtype, tile, was = ledger[k]
        assert was == ""
        b[pos + 4] = 9
        ledger[k] = (pos, size, rtype, tile, "type9")
    return bytes(b), ledger


def expect(ledger, checksums=True):
    """What the inspector reports of a file whose records are the ledger's, by its rules (gvrs_file_inspect.h) and without the library"""
    by_type, bad, records, fails, stop, term, previous_passed = [0] * 7, [], [], 0, END, None, True
    for pos, size, rtype, tile, dmg in ledger:
        if dmg == "type9":
            records.append((pos, size, 9, -1, -1))
            stop, term = BAD_RECORD_TYPE, pos
            break
        checksum = -1
        if checksums:
            checksum = 0 if dmg == "crc" else 1
            if not checksum:
                fails += 1
                if rtype == 2:
                    bad.append(tile)
                if not previous_passed:
                    stop, term = TWO_CHECKSUM_FAILURES, pos
            previous_passed = bool(checksum)
        records.append((pos, size, rtype, tile, checksum))
        by_type[rtype] += 1
        if stop != END:
            break
    if term is None:
        term = ledger[-1][0] + ledger[-1][1]
    return dict(n_records=len(records), n_by_type=by_type, bad_tiles=bad, n_bad_tiles=len(bad), n_checksum_failures=fails, stop=stop,
                termination_pos=term, complete=int(stop == END), failed=int(stop != END or fails != 0), records=records)


def differences(got, want, bad_cap=None, with_records=True):
    """A GvrsInspection against expect()'s answer: the list of what differs"""
    diffs = [(k, getattr(got, k), want[k]) for k in ("n_records", "n_by_type", "n_bad_tiles", "n_checksum_failures", "stop", "termination_pos",
                                                     "complete", "failed") if getattr(got, k) != want[k]]
    if got.bad_tiles != (want["bad_tiles"] if bad_cap is None else want["bad_tiles"][:bad_cap]):
        diffs.append(("bad_tiles", got.bad_tiles[:5], want["bad_tiles"][:5]))
    if with_records and got.records != want["records"]:
        first = None if got.records is None else next((k for k, (r, w) in enumerate(zip(got.records, want["records"])) if r != w), None)
        diffs.append(("records", first))
    return diffs


# ---- the device form's plan restated: anchors and the chain of walks ----------------------------------------------------------------

def model(image, ledger):
    """From the image's directory, the ledger and gf_file_inspect_plan: dict(seg, chunk, n_seg, n_entries, anchors {segment: position},
    first -- the first anchored segment whose walk does not end on a later anchor (k_inspect_chain's F), closes -- whether the walk
    of `first` ends without passing an anchor (no serial walk), walk -- the positions of the records of the structural walk)"""
    f = GvrsFileHip(image)
    seg, chunk, default_room = f.inspect_plan(len(image))
    info, content, n = f.info, content_pos(bool(f.info["checksum_enabled"])), len(image)
    assert content == info["content_pos"]
    n_seg = max(-(-(n - content) // seg), 1)
    nr, nc, w = info["dir_n_rows"], info["dir_n_cols"], 8 if info["dir_extended"] else 4
    raw = np.frombuffer(image, "<u8" if w == 8 else "<u4", nr * nc, info["dir_entries_pos"]).astype(np.uint64)
    p = raw if w == 8 else raw * np.uint64(8)
    k = np.arange(nr * nc)
    tiles = (info["dir_row0"] + k // nc) * N_TILE_COLS + info["dir_col0"] + k % nc
    ok = np.flatnonzero((p != 0) & (p >= content + 8) & (p % np.uint64(8) == 0) & (p <= n - 12))
    words = np.frombuffer(image, "<u4")                              # (every image here is a multiple of 4 long)
    heads = (p[ok].astype(np.int64) - 8) // 4
    ok = ok[((words[heads + 1] & 0xff) == 2) & (words[heads + 2].astype(np.int32) == tiles[ok])]
    places = [content, info["tile_dir_pos"] - 8] + (p[ok].astype(np.int64) - 8).tolist()
    anchors = {}
    for q in places:
        s = (q - content) // seg
        anchors[s] = min(anchors.get(s, q), q)
    walk = []
    for pos, _, _, _, dmg in ledger:
        walk.append(pos)
        if dmg == "type9":
            break
    starts, order = set(walk), sorted(anchors)
    first, closes = order[-1], True
    for s, t in zip(order, order[1:]):
        if anchors[t] not in starts:                                 # (the walk passes it, or stops in front of it)
            first, closes = s, anchors[t] > walk[-1]
            break
    return dict(seg=seg, chunk=chunk, default_room=default_room, n_seg=n_seg, n_entries=nr * nc, anchors=anchors, first=first, closes=closes,
                walk=walk)


# ---- the images --------------------------------------------------------------------------------------------------------------------

def _many_tiles_layout():
    lay = Layout()
    for k in range(3):                                             # (so that a round of 1,024 records holds 511 of the bad tiles, no multiple of 64)
        lay.meta(40, k)
    for t in np.random.default_rng(11).permutation(N_TILES).tolist():
        lay.tile(t)
    return lay


MANY_TILES_RECT = (2, 3, 60, 75)           # the sub-rectangle's directory: 75 columns, no multiple of 64, and 4,500 entries


def many_tiles(variant="sound"):
    """Record k >= 3 is the (k - 3)th tile record of a shuffled order; the directory is record 5,123."""
    if variant == "sound extended":
        return _many_tiles_layout().build(extended=True)
    if variant == "sound sub-rectangle":
        return _many_tiles_layout().build(dir_rect=MANY_TILES_RECT)
    image, ledger = base("many_tiles")
    pairs = {"pair 1023": (1023, 1024), "pair 1024": (1024, 1025), "pair 2047": (2047, 2048), "doubles 2000 and 1100": (2000, 2001, 1100, 1101),
             "doubles 1100 and 2060": (1100, 1101, 2060, 2061)}
    if variant == "sound":
        return image, ledger
    if variant == "every second tile":
        return damaged(image, ledger, crc=range(3, 3 + N_TILES, 2))
    if variant in pairs:
        return damaged(image, ledger, crc=pairs[variant])
    if variant == "double in front of a stop":
        return damaged(image, ledger, crc=(1100, 1101), type9=(3000,))
    if variant == "stop in front of a double":
        return damaged(image, ledger, crc=(3500, 3501), type9=(3000,))
    raise KeyError(variant)


MANY_TILES = ("sound", "sound extended", "sound sub-rectangle", "every second tile", "pair 1023", "pair 1024", "pair 2047", "doubles 2000 and 1100",
              "doubles 1100 and 2060", "double in front of a stop", "stop in front of a double")


def _many_records_layout(n, checksums=True):
    """n records in the walk, the directory the last: 40 tile records, the others metadata records of 16 bytes"""
    tiles_at = {800 * k + 5 for k in range(38)} | {n - 2} | ({CRC_WAVES} if n > CRC_WAVES + 2 else {800 * 38 + 5})
    assert len(tiles_at) == 40 and max(tiles_at) == n - 2
    lay, tile, run = Layout(checksums), 0, 0
    for k in range(n - 1):
        if k in tiles_at:
            lay.meta16(run, k)
            lay.tile(100 * tile + 7)
            tile, run = tile + 1, 0
        else:
            run += 1
    return lay


def many_records(variant="sound"):
    if variant in ("32766", "32767", "32768"):
        return _many_records_layout(int(variant)).build()
    if variant == "checksums off":
        return _many_records_layout(33041, checksums=False).build()
    image, ledger = base("many_records")
    if variant == "sound":
        return image, ledger
    if variant == "fails in front of the seam":                    # (a metadata record, the last of the first turn)
        return damaged(image, ledger, crc=(CRC_WAVES - 1,))
    if variant == "fails behind the seam":                         # (a tile record, the first of the second turn)
        return damaged(image, ledger, crc=(CRC_WAVES,))
    raise KeyError(variant)


MANY_RECORDS = ("sound", "32766", "32767", "32768", "fails in front of the seam", "fails behind the seam", "checksums off")


def _long_span_layout(link=None):
    """Tile records, a free node of 1.5 MiB with a garbage body (segments 2 to 1,538: more than a round of k_inspect_chain without an
    anchor), tile and metadata records up to a metadata record that ends exactly on the seam in front of segment 2,048 -- the
    next round's first segment; seam 1,024 lies inside the free node -- and tile and metadata records behind it.  link: what is
    laid behind segment 1,700, in the chain's second round."""
    lay, tile = Layout(), 0
    for _ in range(30):
        lay.tile(tile)
        tile += 1
    lay.free(3 << 19, garbage=True)
    assert lay.segment() > CHAIN_ROUND + 500
    k, laid = 0, False

    def filler():
        nonlocal tile, k
        lay.tile(tile)
        lay.meta(200 + 8 * (k * 37 % 90), k)
        tile, k = tile + 1, k + 1

    while lay.segment() < 2 * CHAIN_ROUND - 2:
        if link and not laid and lay.segment() >= 1700:
            laid = True
            if link == "size word":
                lay.size_word_too_large(5000)
            else:
                lay.false_anchor(5000)
            continue
        filler()
    lay.to_seam(multiple=CHAIN_ROUND)
    assert lay.segment() == 2 * CHAIN_ROUND
    for _ in range(300):
        filler()
    lay.tile(tile)
    return lay


def long_span(variant="sound"):
    if variant == "sound":
        return _long_span_layout().build()
    if variant == "size word 16 too large":
        return _long_span_layout("size word").build()
    if variant == "false anchor":
        return _long_span_layout("false anchor").build()
    raise KeyError(variant)


LONG_SPAN = ("sound", "size word 16 too large", "false anchor")


def large_sizes(chunk):
    """the four large records' sizes: exactly 1,024 chunks; a chunk and a word more; twice that and a part; the smallest handed on"""
    return [LARGE_WAVES * chunk, LARGE_WAVES * chunk + chunk + 8, (2 * LARGE_WAVES * chunk + 1000 + 7) // 8 * 8, WAVE_CHUNKS * chunk + 8]


LARGE_AT = (3, 7, 11, 15)                  # the large records' numbers: three tile records in front of each


def _large_records_layout():
    chunk = K.plan()[1]
    lay, tile = Layout(), 0
    for k, size in enumerate(large_sizes(chunk)):
        for _ in range(3):
            lay.tile(tile)
            tile += 1
        lay.meta(size, 40 + k)
    for _ in range(3):
        lay.tile(tile)
        tile += 1
    assert [k for k, r in enumerate(lay.ledger) if r[2] == 1] == list(LARGE_AT)
    return lay


def large_records(variant="sound"):
    image, ledger = base("large_records")
    size = {k: ledger[k][1] for k in LARGE_AT}
    where = {"first chunk of the third": (LARGE_AT[2], 100),
             "last whole piece of the first": (LARGE_AT[0], ((size[LARGE_AT[0]] - 4) & ~15) - 3),
             "trailing bytes of the second": (LARGE_AT[1], size[LARGE_AT[1]] - 5),
             "trailing bytes of the first": (LARGE_AT[0], ((size[LARGE_AT[0]] - 4) & ~15) + 1)}
    if variant == "sound":
        return image, ledger
    k, off = where[variant]
    return damaged(image, ledger, crc=(k,), at={k: off})


LARGE_RECORDS = ("sound", "first chunk of the third", "last whole piece of the first", "trailing bytes of the second", "trailing bytes of the first")

N_MANY_LARGE = 1030
_LARGE = {}


def _many_large_items(lay, named):
    """1,030 metadata records of the smallest size that is handed on, a tile record (tiles 0 to 102) behind every tenth"""
    size = WAVE_CHUNKS * K.plan()[1] + 8
    for k in range(N_MANY_LARGE):
        if k not in _LARGE:
            _LARGE[k] = K.other(1, size, 500 + k)
        lay._lay(_LARGE[k], 1)
        if k % 10 == 9:
            lay.tile(k // 10, named)


def _many_large_layout():
    lay = Layout()
    _many_large_items(lay, named=True)
    return lay


def many_large(variant="sound"):
    image, ledger = base("many_large")
    if variant == "sound":
        return image, ledger
    if variant == "two fail":
        large = [k for k, r in enumerate(ledger) if r[2] == 1]
        return damaged(image, ledger, crc=(large[5], large[1027]), at={large[5]: 9000, large[1027]: 16000})
    raise KeyError(variant)


MANY_LARGE = ("sound", "two fail")
WIDE_MARK = 32 << 20                       # 1024 x GF_INSPECT_MAX_SEGMENTS: a span above it has a segment size above the smallest


def _wide_segments_layout():
    """many_large's records, their tile records old copies the directory does not name; then six free nodes of 4 MiB, with garbage
    and with zeros in turn, 120 named tile records behind each (tiles 0 to 719: the second copies among them)"""
    lay = Layout()
    _many_large_items(lay, named=False)
    for g in range(6):
        lay.free((4 << 20) + 8 * g, garbage=g % 2 == 0)
        for t in range(120 * g, 120 * g + 120):
            lay.tile(t)
    return lay


def wide_segments(variant="sound"):
    image, ledger = base("wide_segments")
    if variant == "sound":
        return image, ledger
    if variant == "flipped tile":
        behind = [k for k, r in enumerate(ledger) if r[2] == 2 and r[0] - content_pos() > WIDE_MARK]
        return damaged(image, ledger, crc=(behind[150],))
    raise KeyError(variant)


WIDE_SEGMENTS = ("sound", "flipped tile")

_BASES = {"many_tiles": _many_tiles_layout, "many_records": lambda: _many_records_layout(33041), "large_records": _large_records_layout,
          "many_large": _many_large_layout, "wide_segments": _wide_segments_layout}
_CACHE = {}


def base(family):
    """the family's sound image, built once a session"""
    if family not in _CACHE:
        _CACHE[family] = _BASES[family]().build()
        if family == "wide_segments":
            seg = GvrsFileHip(_CACHE[family][0]).inspect_plan()[0]
            assert seg > MIN_SEGMENT and seg & (seg - 1) != 0 and seg % 8 == 0, seg
    return _CACHE[family]


FAMILIES = {"many_tiles": (many_tiles, MANY_TILES), "many_records": (many_records, MANY_RECORDS), "long_span": (long_span, LONG_SPAN),
            "large_records": (large_records, LARGE_RECORDS), "many_large": (many_large, MANY_LARGE), "wide_segments": (wide_segments, WIDE_SEGMENTS)}
CASES = [(family, variant) for family, (_, variants) in FAMILIES.items() for variant in variants]
_BUILT = {}


def case(family, variant):
    """(image, ledger) of a case.  Images that are laid on their own are kept; a damaged copy of a family's sound image is made anew
    (the 40 MB image twice would be the largest thing the session holds)."""
    if (family, variant) in _BUILT:
        return _BUILT[family, variant]
    got = FAMILIES[family][0](variant)
    if family in ("many_tiles", "many_records", "long_span"):
        _BUILT[family, variant] = got
    return got


def checksums_of(family, variant):
    return variant != "checksums off"
