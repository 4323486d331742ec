"""Test-only: the file images the inspector is held to, shared by tests/test_file_inspect_ref.py (the restatement alone),
tests/test_file_inspect_host.py and tests/test_file_inspect_program.py (gf_file_inspect against it) and
tests/test_gpu_file_inspect.py (gf_file_inspect_dev against gf_file_inspect).  Tiles of 4 x 4 int cells as standard-form records
(88 bytes: exactly the largest a tile record may have), so no codec is involved.  A LAYOUT is the file's content in file order:
  ("t", tile)          a tile record the directory names         ("u", tile, seed)   one it does not name (an old copy)
  ("big", tile)        a named tile record 8 bytes too large      ("m", size, seed)   a metadata record of `size` bytes
  ("f", size)          a free node, its body zeros                ("g", size)         a free node whose body is garbage
  ("seam",)            a metadata record that ends exactly on the next segment seam
  ("fake", tile)       a metadata record whose body holds, 16 bytes in, what looks like the head of a record of `tile`
The sizes that matter -- segment, CRC chunk, chunks a wave takes -- come from gf_file_inspect_plan, never from here."""
import struct

import numpy as np

import gvrs_file_build as B
import gvrs_inspect_ref as R
import file_update_cases as U
from gridfour_amd import GvrsFileHip

GRID = (24, 32, 4, 4)                      # 6 x 8 tiles of 4 x 4 cells
N_TILES = 48
ELEMENTS = [B.element("z", "int")]
WAVE_CHUNKS = 8                            # a record of more chunks than this is checksummed chunk by chunk (gvrs_file_inspect.h)


_PLAN = []


def plan():
    """(segment bytes, CRC chunk bytes) of an image of these sizes"""
    if _PLAN:
        return _PLAN[0]
    f = GvrsFileHip(B.build_image(GRID, ELEMENTS, {0: tile_record(0)})[0])
    seg, chunk, _ = f.inspect_plan(6000)
    _PLAN.append((seg, chunk))
    return seg, chunk


def tile_record(tile, checksums=True, seed=0, extra=0):
    cells = (np.arange(16, dtype=np.int32) * 3 + tile * 7 + seed).reshape(4, 4)
    if not extra:
        return B.standard_record(tile, [cells], checksums)
    return B.frame_record(tile, [cells.tobytes() + b"\1" * extra], checksums)


def with_crc(rec, checksums=True, head_only=False):
    b = bytearray(rec)
    struct.pack_into("<I", b, len(b) - 4, (R.crc32c(b[:8]) if head_only else R.crc32c(b[:-4])) if checksums else 0)
    return bytes(b)


def other(rtype, size, seed, checksums=True):
    assert size % 8 == 0 and size >= 16
    return with_crc(B.other_record(rtype, size - 8, seed), checksums)


def free_node(size, checksums=True, garbage=False):
    body = np.random.default_rng(size).integers(1, 256, size - 12, dtype=np.uint8).tobytes() if garbage else b"\0" * (size - 12)
    return with_crc(struct.pack("<ii", size, 0) + body + b"\0" * 4, checksums, head_only=True)


def make(layout, checksums=True, extended=False, overrides=None, tail=b""):
    """-> the image.  overrides: {tile: ("fake", k)} points the tile's entry at the k-th fake head, {tile: ("mid", other tile)} into
    the middle of the other tile's record."""
    seg = plan()[0]
    content = len(B.header_record(GRID, ELEMENTS, (), checksums))
    records, order, gaps, pending, at, fakes = {}, [], {}, b"", content, []
    for item in layout:
        kind = item[0]
        if kind in ("t", "big"):
            records[item[1]] = tile_record(item[1], checksums, extra=8 if kind == "big" else 0)
            gaps[len(order)] = pending
            order.append(item[1])
            at += len(records[item[1]])
            pending = b""
            continue
        if kind == "u":
            rec = tile_record(item[1], checksums, seed=item[2])
        elif kind == "m":
            rec = other(1, item[1], item[2], checksums)
        elif kind in ("f", "g"):
            rec = free_node(item[1], checksums, kind == "g")
        elif kind == "seam":
            size = seg - (at - content) % seg
            rec = other(1, size if size >= 16 else size + seg, 99, checksums)
        elif kind == "fake":
            b = bytearray(B.other_record(1, 200 - 8, item[1]))
            struct.pack_into("<iii", b, 16, 88, 2, item[1])
            rec = with_crc(bytes(b), checksums)
            fakes.append(at + 16)
        pending += rec
        at += len(rec)
    assert not pending, "a layout ends with a named tile record (the directory follows)"
    image, positions = B.build_image(GRID, ELEMENTS, records, (), checksums, order=order, between=lambda k: gaps[k], extended=extended)
    if overrides:
        raw = {}
        for tile, (what, k) in overrides.items():
            p = fakes[k] + 8 if what == "fake" else positions[k] + 24
            raw[tile] = p if extended else p // 8
        image, _ = B.build_image(GRID, ELEMENTS, records, (), checksums, order=order, between=lambda k: gaps[k], extended=extended,
                                 entry_overrides=raw)
    return image + tail


def shuffled_layout(n=40, seed=5):
    """tile records in shuffled order, metadata records and free nodes between them"""
    tiles = np.random.default_rng(seed).permutation(N_TILES)[:n].tolist()
    layout = []
    for k, t in enumerate(tiles):
        if k % 7 == 3:
            layout.append(("m", 40 + 8 * (k % 5), k))
        if k % 9 == 4:
            layout.append(("f", 32 + 8 * (k % 4)))
        layout.append(("t", t))
    return layout


def sound_cases():
    """name -> image: every one passes and is complete, unless the name says what is listed"""
    seg, chunk = plan()
    asc = [("t", t) for t in range(N_TILES)]
    big = WAVE_CHUNKS * chunk
    cases = {
        "compact": make(asc),
        "extended": make(asc, extended=True),
        "shuffled": make(shuffled_layout()),
        "shuffled extended": make(shuffled_layout(), extended=True),
        "starts on a seam": make(asc[:5] + [("seam",)] + asc[5:20] + [("seam",)] + asc[20:]),
        "long metadata": make(asc[:3] + [("m", 2 * seg + 200, 1)] + asc[3:]),
        "long free node": make(asc[:3] + [("g", 2 * seg + 200)] + asc[3:]),
        "long both": make(asc[:3] + [("m", 2 * seg + 64, 1), ("f", 3 * seg)] + asc[3:30] + [("f", 2 * seg + 8)] + asc[30:]),
        "unnamed in front of the anchor": make(asc[:5] + [("seam",), ("u", 40, 1), ("u", 41, 2), ("m", 48, 3), ("u", 40, 4)] + asc[5:30]),
        "metadata of whole chunks": make(asc[:4] + [("m", big + chunk, 7)] + asc[4:]),
        "metadata of chunks and a word": make(asc[:4] + [("m", big + chunk + 8, 7)] + asc[4:]),
        "metadata of chunks and a part": make(asc[:4] + [("m", big + chunk + 1000, 7), ("m", big + 8, 8)] + asc[4:]),
        "metadata one wave takes": make(asc[:4] + [("m", big, 7)] + asc[4:]),
        "garbage in a free node": make(asc[:10] + [("g", 400)] + asc[10:]),
        "old copy": make(asc[:10] + [("u", 3, 9)] + asc[10:]),
        "no checksums": make(shuffled_layout(), checksums=False),
        "no checksums long": make(asc[:3] + [("m", 2 * seg + 64, 1), ("g", 3 * seg)] + asc[3:], checksums=False),
        "bytes behind the last record": make(shuffled_layout(), tail=b"\7" * 8),
        "false anchor": make(asc[:12] + [("m", 600, 2), ("fake", 47), ("m", 800, 3)] + asc[12:40], overrides={47: ("fake", 0)}),
        "false anchor extended": make(asc[:12] + [("fake", 47), ("m", 1800, 3)] + asc[12:40], extended=True, overrides={47: ("fake", 0)}),
        "entry into the middle of a record": make(asc[:40], overrides={20: ("mid", 20)}),
        "one tile": make([("t", 17)]),
    }
    # file_update_cases' images, every record of the standard form's size (its own are larger: the inspector calls them invalid)
    small = [(k[0], k[1], 40) if k[0] == "t" else k for k in U.BASE]
    cases["free space directory"] = U.make_file(small)
    records, tiles = U.writes_of([(1, 0), (50, 40), (3, 0), (60, 40)])
    cases["updated"] = U.model(U.make_file(small), records, tiles)[0]
    return cases


def records_of(image):
    f = GvrsFileHip(image)
    return R.inspect(image, R.facts_of(f))["records"]


def patched(image, at, data):
    b = bytearray(image)
    b[at:at + len(data)] = data
    return bytes(b)


def flipped(image, at):
    return patched(image, at, bytes([image[at] ^ 0x40]))


def damaged_cases():
    """name -> image, one damage each unless the name says otherwise"""
    base = make(shuffled_layout())
    recs = records_of(base)
    kinds = [r[2] for r in recs]

    def pair(a, b, start=0):
        """the first k >= start with records k, k + 1 of types a, b"""
        return next(k for k in range(start, len(recs) - 1) if kinds[k] == a and kinds[k + 1] == b)

    def body(k):
        return recs[k][0] + 16                                     # (a tile record's first cell, a metadata record's content)

    def size_word(k, value):
        return patched(base, recs[k][0], struct.pack("<i", value))

    tt, tm, mt = pair(2, 2), pair(2, 1), pair(1, 2)
    meta = kinds.index(1)
    free = kinds.index(0)
    late = pair(2, 2, len(recs) // 2)
    cases = {
        "flipped tile": flipped(base, body(tt)),
        "tile and tile": flipped(flipped(base, body(tt)), body(tt + 1)),
        "tile and metadata": flipped(flipped(base, body(tm)), body(tm + 1)),
        "metadata and tile": flipped(flipped(base, body(mt)), body(mt + 1)),
        "three in a row": flipped(flipped(flipped(base, body(tt)), body(tt + 1)), body(tt + 2)),
        "a good record between": flipped(flipped(base, body(tt)), body(tt + 2)),
        "tile directory fails": flipped(base, len(base) - 2),
        "tile directory body": flipped(base, recs[-1][0] + 10),    # (a reserved byte behind the extended flag: no entry changes)
        "free head fails": flipped(base, recs[free][0] + 6),
        "free checksum word": flipped(base, recs[free][0] + recs[free][1] - 1),
        "tile index -1": patched(base, recs[tt][0] + 8, struct.pack("<i", -1)),
        "tile index = count": patched(base, recs[tt][0] + 8, struct.pack("<i", N_TILES)),
        "tile too large": make([("t", t) for t in range(20)] + [("big", 20)] + [("t", t) for t in range(21, 40)]),
        "type 7": patched(base, recs[late][0] + 4, b"\7"),
        "type 255": patched(base, recs[meta][0] + 4, b"\xff"),
        "zero size": size_word(late, 0),
        "size -8": size_word(late, -8),
        "size 8": size_word(meta, 8),
        "size 20": size_word(late, 20),
        "size past the image": size_word(meta, 1 << 20),
        "large tile past the image": size_word(len(recs) - 2, 1 << 12),
        "size into the next record": size_word(meta, recs[meta][1] + 24),
        "size over the next record": size_word(meta, recs[meta][1] + recs[meta + 1][1]),
        "stop in front of a double": patched(flipped(flipped(base, body(late)), body(late + 1)), recs[tt][0] + 4, b"\x09"),
        "double in front of a stop": patched(flipped(flipped(base, body(tt)), body(tt + 1)), recs[late][0] + 4, b"\x09"),
        "first record": patched(base, recs[0][0] + 4, b"\x08"),
    }
    # an old copy that fails: listed, the walk complete
    old = make([("t", t) for t in range(10)] + [("u", 3, 9)] + [("t", t) for t in range(10, 30)])
    k = next(i for i, r in enumerate(records_of(old)) if r[2] == 2 and r[3] == 3 and i > 5)
    cases["old copy fails"] = flipped(old, records_of(old)[k][0] + 20)
    # the link that does not close and rejoins: a size word 16 too large lands on what looks like a record that ends with its host
    asc = [("t", t) for t in range(N_TILES)]
    for name, checksums in (("rejoins", True), ("rejoins without checksums", False)):
        image = make(asc[:14] + [("m", 64, 1), ("fake", 2)] + asc[14:40], checksums=checksums)
        r2 = records_of(image)
        m = next(i for i, r in enumerate(r2) if r[2] == 1)
        image = patched(image, r2[m][0], struct.pack("<i", 64 + 16))
        cases[name] = patched(image, r2[m + 1][0] + 16, struct.pack("<ii", 200 - 16, 1))       # (the fake head: a metadata record to the host's end)
    cases["no checksums, past the image"] = patched(make(shuffled_layout(), checksums=False), recs[meta][0], struct.pack("<i", 1 << 20))
    cases["no checksums, flipped"] = flipped(make(shuffled_layout(), checksums=False), body(tt))
    return cases


_CACHE = {}


def all_cases():
    """name -> image, sound and damaged; built once"""
    if not _CACHE:
        _CACHE.update({"sound: " + k: v for k, v in sound_cases().items()})
        _CACHE.update({"damaged: " + k: v for k, v in damaged_cases().items()})
    return _CACHE
