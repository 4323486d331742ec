"""Test-only reference for the file writers (gf_file_assemble, gf_file_write_block_elems[_dev]): a file's facts in one Python
description from which both the library's GvrsFileFacts and a whole image in pure Python follow -- the header record by
gvrs_file_build.header_record, every other record framed here as gvrs_file_build.frame_record frames a tile's (size a multiple of
8, type, zeros, CRC-32C), the metadata records and the metadata directory that gvrs_file_build lacks, and the tile directory over
the bounding rectangle of the tiles that have a record.  sample_spec() takes one of the reference's files apart into the same
description: what gf_file_info does not carry (ranges, labels, UUID, time modified, the metadata records) is read from its bytes."""
import struct

import numpy as np

import gridfour_amd
from gridfour_amd import GvrsFileFacts, GvrsFileHip

import gvrs_file_build as B

RECORD_METADATA_DIR = 4
KIND_OF_CODE = {v: k for k, v in B.TYPE_CODES.items()}


def spec(grid, elements, codec_ids=(), checksums=True, metadata=(), **header_facts):
    """A file's facts: grid = (rows, columns of the grid, rows, columns of a tile); elements: gvrs_file_build.element dicts (an "icf"
    element may carry vmin_f / vmax_f, the float range the header states; default: the codes' range as values, in float32);
    metadata: (name, record id, type code, content bytes, description) per record; header_facts: what gvrs_file_build.header_record
    takes of uuid, time_modified, raster_space, coordinate_system, domain, cell_size, m2r, r2m, product_label."""
    return dict(grid=tuple(grid), elements=list(elements), codec_ids=list(codec_ids), checksums=bool(checksums), metadata=list(metadata),
                header_facts=dict(header_facts))


def icf_float_range(el):
    if "vmin_f" in el:
        return np.float32(el["vmin_f"]), np.float32(el["vmax_f"])
    scale, offset = np.float32(el["scale"]), np.float32(el["offset"])
    return np.float32(el["vmin"]) / scale + offset, np.float32(el["vmax"]) / scale + offset


def lib_facts(s):
    """The GvrsFileFacts of a spec"""
    elems, fills, facts = [], [], []
    for el in s["elements"]:
        d = dict(name=el["name"], label=el["label"], description=el["description"], unit=el["unit"], continuous=el["continuous"])
        if el["kind"] == "icf":
            elems.append(("icf", el["scale"], el["offset"], el["fill"], el["fill_f"]))
            fills.append(None)
            d["range"] = icf_float_range(el) + (el["vmin"], el["vmax"])
        else:
            elems.append(el["kind"])
            fills.append(el["fill"])
            d["range"] = (el["vmin"], el["vmax"])
        facts.append(d)
    h = s["header_facts"]
    kw = {k: h[k] for k in ("raster_space", "coordinate_system", "cell_size", "m2r", "r2m", "product_label", "uuid", "time_modified") if k in h}
    if "domain" in h:
        kw["bounds"] = h["domain"]
    return GvrsFileFacts(s["grid"], elems, fills=fills, elem_facts=facts, codec_ids=s["codec_ids"], checksums=s["checksums"], metadata=s["metadata"], **kw)


def _utf(b):
    b = b if isinstance(b, bytes) else b.encode()
    return struct.pack("<H", len(b)) + b


def frame(rtype, content, checksums):
    """Any record around its content: [size][type 0 0 0][content][zeros][CRC-32C | 0], size = multipleOf8(content + 12)"""
    size = (8 + len(content) + 4 + 7) // 8 * 8
    rec = bytearray(struct.pack("<i", size) + bytes([rtype, 0, 0, 0]) + bytes(content))
    rec += b"\0" * (size - len(rec))
    if checksums:
        struct.pack_into("<I", rec, size - 4, B.crc32c(rec[:size - 4]))
    return bytes(rec)


def metadata_record(m, checksums):
    name, record_id, type_code, content, description = m
    return frame(B.RECORD_METADATA, _utf(name) + struct.pack("<i", record_id) + bytes([type_code, 0, 0, 0]) + struct.pack("<i", len(content)) +
                 bytes(content) + _utf(description), checksums)


def header(s, **positions):
    elements = []
    for el in s["elements"]:
        elements.append(el)
    return B.header_record(s["grid"], elements, s["codec_ids"], s["checksums"], **positions, **s["header_facts"])


def ref_image(s, records, extended=False):
    """The whole image in Python: records = (tile index, record bytes) in the order they are laid; b"" gets no place.  Extended only
    when asked for (no test image reaches 1 << 35)."""
    grid, checks = s["grid"], s["checksums"]
    n_tile_cols = -(-grid[1] // grid[3])
    front = bytearray(header(s))
    meta_positions = []
    for m in s["metadata"]:
        meta_positions.append(len(front) + 8)
        front += metadata_record(m, checks)
    body, positions = bytearray(), {}
    for t, rec in records:
        if len(rec):
            assert t not in positions
            positions[t] = len(front) + len(body) + 8
            body += rec
    records_end = len(front) + len(body)
    meta_dir = b""
    if s["metadata"]:
        content = struct.pack("<i", len(s["metadata"]))
        for m, p in zip(s["metadata"], meta_positions):
            content += struct.pack("<q", p) + _utf(m[0]) + struct.pack("<i", m[1]) + bytes([m[2]])
        meta_dir = frame(RECORD_METADATA_DIR, content, checks)
    if positions:
        rows, cols = [t // n_tile_cols for t in positions], [t % n_tile_cols for t in positions]
        r0, c0, nr, nc = min(rows), min(cols), max(rows) - min(rows) + 1, max(cols) - min(cols) + 1
    else:
        r0 = c0 = nr = nc = 0
    entries = b""
    for r in range(r0, r0 + nr):
        for c in range(c0, c0 + nc):
            p = positions.get(r * n_tile_cols + c, 0)
            entries += struct.pack("<q", p) if extended else struct.pack("<I", p // 8)
    tile_dir = frame(B.RECORD_TILE_DIR, bytes([0, 1 if extended else 0]) + b"\0" * 6 + struct.pack("<iiii", r0, c0, nr, nc) + entries, checks)
    head = header(s, metadata_dir_pos=records_end + 8 if meta_dir else 0, tile_dir_pos=records_end + len(meta_dir) + 8)
    assert len(head) == len(front) - sum(len(metadata_record(m, checks)) for m in s["metadata"])
    return head + bytes(front[len(head):]) + bytes(body) + meta_dir + tile_dir


class _Cursor:
    def __init__(self, data, pos):
        self.d, self.p = data, pos

    def take(self, fmt):
        v = struct.unpack_from("<" + fmt, self.d, self.p)
        self.p += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def utf(self):
        n = self.take("H")
        self.p += n
        return self.d[self.p - n:self.p].decode()

    def align4(self):
        self.p += -self.p & 3


def sample_spec(path):
    """One of the reference's files -> (its spec, its tile records as (tile index, bytes) in file order)"""
    data = open(path, "rb").read()
    f = GvrsFileHip(data)
    i = f.info
    c = _Cursor(data, 104 + 16 + 8 + 8 + 48 + 96 + 4)
    elements = []
    for e in range(i["n_elems"]):
        code, continuous = c.take("BB")
        c.p += 6
        name = c.utf()
        c.align4()
        kind = KIND_OF_CODE[code]
        kw = {}
        if kind == "int":
            vmin, vmax, fill = c.take("iii")
        elif kind == "short":
            vmin, vmax, fill = c.take("hhh")
        elif kind == "float":
            vmin, vmax, fill = c.take("fff")
        else:
            vmin_f, vmax_f, fill_f, scale, offset = c.take("fffff")
            vmin, vmax, fill = c.take("iii")
            kw = dict(scale=scale, offset=offset, fill_f=fill_f, vmin_f=vmin_f, vmax_f=vmax_f)
        label, description, unit = c.utf(), c.utf(), c.utf()
        c.align4()
        el = B.element(name, kind, fill=fill, vmin=vmin, vmax=vmax, label=label, description=description, unit=unit, continuous=bool(continuous),
                       **{k: v for k, v in kw.items() if k in ("scale", "offset", "fill_f")})
        el.update({k: v for k, v in kw.items() if k in ("vmin_f", "vmax_f")})
        elements.append(el)
    metadata = []
    if i["metadata_dir_pos"]:
        m = _Cursor(data, i["metadata_dir_pos"])
        for _ in range(m.take("i")):
            pos = m.take("q")
            m.utf()
            m.p += 5
            r = _Cursor(data, pos)
            name, record_id, type_code = r.utf(), r.take("i"), r.take("B")
            r.p += 3
            n = r.take("i")
            content = data[r.p:r.p + n]
            r.p += n
            metadata.append((name, record_id, type_code, content, r.utf()))
    n_tiles = -(-f.grid[0] // f.grid[2]) * -(-f.grid[1] // f.grid[3])
    at = sorted((f.tile_position(t), t) for t in range(n_tiles) if f.tile_position(t))
    records = [(t, data[p - 8:p - 8 + struct.unpack_from("<i", data, p - 8)[0]]) for p, t in at]
    s = spec(f.grid, elements, i["codec_ids"], i["checksum_enabled"], metadata, uuid=data[24:40], time_modified=struct.unpack_from("<q", data, 40)[0],
             raster_space=i["raster_space"], coordinate_system=i["coordinate_system"], domain=(i["x0"], i["y0"], i["x1"], i["y1"]),
             cell_size=(i["cell_size_x"], i["cell_size_y"]), m2r=tuple(i["m2r"]), r2m=tuple(i["r2m"]), product_label=i["product_label"])
    f.close()
    return s, records, data


def elems_of(s):
    """The spec's elements as the record calls of CodecMasterHip take them, and their fills"""
    elems, fills = [], []
    for el in s["elements"]:
        elems.append(("icf", el["scale"], el["offset"], el["fill"], el["fill_f"]) if el["kind"] == "icf" else el["kind"])
        fills.append(None if el["kind"] == "icf" else el["fill"])
    return elems, fills


KINDS = {"GvrsHuffman": gridfour_amd.CODEC_HUFFMAN, "GvrsDeflate": gridfour_amd.CODEC_DEFLATE, "GvrsFloat": gridfour_amd.CODEC_NONE,
         "GvrsCanonicalHuffman": gridfour_amd.CODEC_CANON_HUFFMAN, "LSOP12": gridfour_amd.CODEC_LSOP12, "LSOP08": gridfour_amd.CODEC_LSOP08}
