"""Test-only writer of GVRS 1.04 file images (the layout gf_file_open reads, include/gvrs_hip_codec.h): a header record with a
correct CRC-32C, any element list and codec ids, records in any order with other records and junk between them, and a compact
or extended tile directory over any sub-rectangle of the tiles.  header_record() reproduces the header record of the
reference's Sample01_IntNoComp.gvrs byte for byte from that file's facts (tests/test_file_open.py), which keeps it honest."""
import ctypes as C
import struct

import numpy as np

from gridfour_amd._lib import lib

TYPE_CODES = {"int": 0, "icf": 1, "float": 2, "short": 3}          # GvrsElementType code values: not the GF_ELEM_* numbers
RECORD_TILE, RECORD_TILE_DIR, RECORD_METADATA, RECORD_HEADER = 2, 5, 1, 6
STANDARD_IDS = ("GvrsHuffman", "GvrsDeflate", "GvrsFloat")


def crc32c(data):
    data = bytes(data)
    return lib().gf_crc32c(C.c_char_p(data), len(data))


def _utf(s):
    b = s.encode()
    return struct.pack("<H", len(b)) + b


def _pad4(buf):
    buf += b"\0" * (-len(buf) & 3)


def element(name, kind, fill=None, vmin=None, vmax=None, scale=1.0, offset=0.0, fill_f=float("nan"), label="", description="", unit="",
            continuous=False):
    """One element's facts.  kind: "int" | "short" | "float" | "icf"; fill: the fill value (an icf's is its code, fill_f its value)."""
    defaults = {"int": (-2 ** 31, -2 ** 31 + 1, 2 ** 31 - 1), "short": (-32768, -32767, 32767), "float": (float("nan"), float("-inf"), float("inf")),
                "icf": (-2 ** 31, -2 ** 31 + 1, 2 ** 31 - 1)}[kind]
    return dict(name=name, kind=kind, fill=defaults[0] if fill is None else fill, vmin=defaults[1] if vmin is None else vmin,
                vmax=defaults[2] if vmax is None else vmax, scale=scale, offset=offset, fill_f=fill_f, label=label, description=description,
                unit=unit, continuous=continuous)


def header_record(grid, elements, codec_ids=(), checksums=True, tile_dir_pos=0, metadata_dir_pos=0, freespace_dir_pos=0, uuid=b"\0" * 16,
                  time_modified=0, time_opened=0, n_levels=1, raster_space=0, coordinate_system=0, domain=None, cell_size=(1.0, 1.0),
                  m2r=(1.0, 0.0, -0.0, 0.0, 1.0, -0.0), r2m=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0), product_label="", version=(1, 4), size=None,
                  type_codes=None):
    """The bytes [0, content_pos) of a file: the file head and the header record.  grid = (rows, columns of the grid, rows, columns of
    a tile); size: the header record's size (default: the smallest multiple of 8 with 8 spare bytes in front of the checksum);
    type_codes: per element another type code than its kind's (a refusal case)."""
    nr, nc = grid[0], grid[1]
    domain = (0.0, 0.0, float(nc - 1), float(nr - 1)) if domain is None else domain
    b = bytearray(b"gvrs raster\0" + bytes([version[0], version[1], 0, 0]))
    b += struct.pack("<i", 0) + bytes([RECORD_HEADER, 0, 0, 0]) + bytes(uuid)
    b += struct.pack("<qqqq", time_modified, time_opened, freespace_dir_pos, metadata_dir_pos)
    b += struct.pack("<h", n_levels) + b"\0" * 6 + struct.pack("<q", tile_dir_pos) + b"\0" * 16
    assert len(b) == 104
    b += struct.pack("<iiii", *grid) + b"\0" * 8
    b += bytes([1 if checksums else 0, raster_space, coordinate_system]) + b"\0" * 5
    b += struct.pack("<6d", *domain, *cell_size) + struct.pack("<6d", *m2r) + struct.pack("<6d", *r2m)
    b += struct.pack("<i", len(elements))
    for e, el in enumerate(elements):
        code = TYPE_CODES[el["kind"]] if type_codes is None else type_codes[e]
        b += bytes([code, 1 if el["continuous"] else 0]) + b"\0" * 6 + _utf(el["name"])
        _pad4(b)
        if el["kind"] == "short":
            b += struct.pack("<hhh", el["vmin"], el["vmax"], el["fill"])
        elif el["kind"] == "float":
            b += struct.pack("<fff", el["vmin"], el["vmax"], el["fill"])
        elif el["kind"] == "icf":
            b += struct.pack("<fffff", el["vmin"] / el["scale"] + el["offset"], el["vmax"] / el["scale"] + el["offset"], el["fill_f"],
                             el["scale"], el["offset"])
            b += struct.pack("<iii", el["vmin"], el["vmax"], el["fill"])
        else:
            b += struct.pack("<iii", el["vmin"], el["vmax"], el["fill"])
        b += _utf(el["label"]) + _utf(el["description"]) + _utf(el["unit"])
        _pad4(b)
    b += struct.pack("<i", len(codec_ids))
    for cid in codec_ids:
        b += _utf(cid)
    b += _utf(product_label)
    if size is None:
        size = (len(b) - 16 + 8 + 4 + 7) // 8 * 8
    assert 16 + size - 4 >= len(b), "the header record's size does not hold its fields"
    b += b"\0" * (16 + size - len(b))
    struct.pack_into("<i", b, 16, size)
    if checksums:
        struct.pack_into("<I", b, 16 + size - 4, crc32c(b[16:16 + size - 4]))
    return bytes(b)


def refresh_header_crc(image):
    """The image with its header record's checksum computed anew (after a field was changed on purpose)."""
    b = bytearray(image)
    (size,) = struct.unpack_from("<i", b, 16)
    struct.pack_into("<I", b, 16 + size - 4, crc32c(b[16:16 + size - 4]))
    return bytes(b)


def frame_record(tile_index, payloads, checksum=True, rtype=RECORD_TILE):
    """A tile record around its elements' bytes (standard form or packings): [size][type 0 0 0][tile index]{[n][n bytes]}[zeros][CRC-32C | 0]"""
    body = struct.pack("<i", tile_index) + b"".join(struct.pack("<i", len(p)) + bytes(p) for p in payloads)
    size = (8 + len(body) + 4 + 7) // 8 * 8
    rec = bytearray(struct.pack("<i", size) + bytes([rtype, 0, 0, 0]) + body)
    rec += b"\0" * (size - len(rec))
    if checksum:
        struct.pack_into("<I", rec, size - 4, crc32c(rec[:size - 4]))
    return bytes(rec)


def refresh_record_crc(image, position):
    """The image with the checksum of the record whose content lies at `position` computed anew."""
    b = bytearray(image)
    (size,) = struct.unpack_from("<i", b, position - 8)
    struct.pack_into("<I", b, position - 8 + size - 4, crc32c(b[position - 8:position - 8 + size - 4]))
    return bytes(b)


def standard_record(tile_index, tiles, checksum=True):
    """A standard-form record: tiles = per element the tile's cells as a numpy array of the stored type (int32 / int16 / float32)"""
    payloads = []
    for t in tiles:
        raw = np.ascontiguousarray(t).tobytes()
        payloads.append(raw + b"\0" * (-len(raw) & 3))
    return frame_record(tile_index, payloads, checksum)


def other_record(rtype, n_bytes, seed=0):
    """A record of another type (metadata, free space) of about n_bytes of arbitrary content"""
    size = (8 + n_bytes + 7) // 8 * 8
    rng = np.random.default_rng(seed)
    return struct.pack("<i", size) + bytes([rtype, 0, 0, 0]) + rng.integers(0, 256, size - 8, dtype=np.uint8).tobytes()


def build_image(grid, elements, records, codec_ids=(), checksums=True, order=None, between=None, dir_rect=None, extended=False,
                entry_overrides=None, **header_facts):
    """A whole file image.  records: {tile index: record bytes}; order: the tile indices in the order their records are laid
    (default: ascending); between(k): bytes to lay in front of the k-th record (a multiple of 8 long: other records, junk);
    dir_rect = (row0, col0, n_rows, n_cols): the directory's rectangle of tiles (default: all of them; tiles outside it are not
    named even where a record is laid); entry_overrides: {tile index: the raw entry value to write instead}.
    Returns (image, positions {tile index: the position its directory entry names})."""
    n_tile_rows, n_tile_cols = -(-grid[0] // grid[2]), -(-grid[1] // grid[3])
    dir_rect = (0, 0, n_tile_rows, n_tile_cols) if dir_rect is None else dir_rect
    probe = header_record(grid, elements, codec_ids, checksums, **header_facts)
    body = bytearray()
    positions = {}
    order = sorted(records) if order is None else order
    for k, t in enumerate(order):
        if between is not None:
            junk = between(k)
            assert len(junk) % 8 == 0
            body += junk
        positions[t] = len(probe) + len(body) + 8
        body += records[t]
        assert len(body) % 8 == 0
    tile_dir_pos = len(probe) + len(body) + 8
    r0, c0, nr, nc = dir_rect
    entries = bytearray()
    for r in range(r0, r0 + nr):
        for c in range(c0, c0 + nc):
            t = r * n_tile_cols + c
            p = positions.get(t, 0)
            if entry_overrides and t in entry_overrides:
                raw = entry_overrides[t]
            else:
                raw = p if extended else p // 8
            entries += struct.pack("<q", raw) if extended else struct.pack("<I", raw & 0xffffffff)
    content = bytes([0, 1 if extended else 0]) + b"\0" * 6 + struct.pack("<iiii", r0, c0, nr, nc) + bytes(entries)
    size = (8 + len(content) + 4 + 7) // 8 * 8
    directory = bytearray(struct.pack("<i", size) + bytes([RECORD_TILE_DIR, 0, 0, 0]) + content)
    directory += b"\0" * (size - len(directory))
    if checksums:
        struct.pack_into("<I", directory, size - 4, crc32c(directory[:size - 4]))
    head = header_record(grid, elements, codec_ids, checksums, tile_dir_pos=tile_dir_pos, **header_facts)
    assert len(head) == len(probe)
    named = {t: p for t, p in positions.items() if r0 <= t // n_tile_cols < r0 + nr and c0 <= t % n_tile_cols < c0 + nc}
    return head + bytes(body) + bytes(directory), named


def entry_offset(image, info, tile_index):
    """Where in the image the directory entry of a tile lies (info: GvrsFileHip.info), and its width in bytes"""
    n_tile_cols = -(-info["grid"][1] // info["grid"][3])
    k = (tile_index // n_tile_cols - info["dir_row0"]) * info["dir_n_cols"] + (tile_index % n_tile_cols - info["dir_col0"])
    w = 8 if info["dir_extended"] else 4
    return info["dir_entries_pos"] + k * w, w
