"""gf_file_open and its getters without a GPU: the reference's fifteen sample files opened as files (header record, specification,
tile directory, every tile's position), the test-only writer gvrs_file_build.py held to the reference's own header bytes, every
refusal of gf_file_open on images that writer makes, damaged and truncated samples, and the parser alone under the sanitizers
(tests/csrc/file_parse_test.cpp)."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import gridfour_amd
from gridfour_amd import GvrsFileHip, GvrsHipError
from gridfour_amd import _lib

import gvrs_file_build as B

HERE = os.path.dirname(os.path.abspath(__file__))
INT_MIN = -2 ** 31
NAN = float("nan")
STD = ["GvrsHuffman", "GvrsDeflate", "GvrsFloat"]
STD_KINDS = [gridfour_amd.CODEC_HUFFMAN, gridfour_amd.CODEC_DEFLATE, gridfour_amd.CODEC_NONE]
SAMPLES = ["Sample00_ShortNoComp", "Sample01_IntNoComp", "Sample02_FltNoComp", "Sample03_ICFNoComp", "Sample04_ShortComp", "Sample05_IntComp",
           "Sample06_FltComp", "Sample07_ICFComp", "Sample08_MixedTypes", "Sample09_ShortNoComp", "Sample10_IntNoComp", "Sample11_FltNoComp",
           "Sample12_ICFNoComp", "Sample13_ModelCoord", "Sample14_LSOP"]
SRT, INT, FLT = ("zSrt", "short", -32768), ("zInt", "int", INT_MIN), ("zFlt", "float", NAN)
ICF = ("zIcf", "icf", INT_MIN, 1.0, 0.0, NAN)
# per sample: grid, checksums, elements (name, kind, fill[, scale, offset, fill_f]), codec ids, content / directory position,
# the directory's rectangle, the position of every tile (tile 0 first)
FACTS = {
    0: ((10, 10, 5, 5), 1, [SRT], [], 376, 1184, (0, 0, 2, 2), [1024, 952, 880, 808]),
    1: ((10, 10, 5, 5), 1, [INT], [], 384, 1384, (0, 0, 2, 2), [1176, 1056, 936, 816]),
    2: ((10, 10, 5, 5), 1, [FLT], [], 384, 1384, (0, 0, 2, 2), [1176, 1056, 936, 816]),
    3: ((10, 10, 5, 5), 1, [ICF], [], 448, 1448, (0, 0, 2, 2), [1240, 1120, 1000, 880]),
    4: ((100, 100, 50, 50), 1, [SRT], STD, 408, 1184, (0, 0, 2, 2), [1032, 968, 904, 840]),
    5: ((100, 100, 50, 50), 1, [INT], STD, 416, 1192, (0, 0, 2, 2), [1040, 976, 912, 848]),
    6: ((100, 100, 50, 50), 1, [FLT], STD, 416, 2216, (0, 0, 2, 2), [1760, 1424, 1136, 848]),
    7: ((100, 100, 50, 50), 1, [ICF], STD, 480, 1256, (0, 0, 2, 2), [1104, 1040, 976, 912]),
    8: ((10, 10, 5, 5), 0, [SRT, FLT], [], 416, 1640, (0, 0, 2, 2), [1376, 1200, 1024, 848]),
    9: ((10, 10, 6, 6), 1, [SRT], [], 376, 1280, (0, 0, 2, 2), [1096, 1000, 904, 808]),
    10: ((10, 10, 6, 6), 1, [INT], [], 384, 1576, (0, 0, 2, 2), [1320, 1152, 984, 816]),
    11: ((10, 10, 6, 6), 1, [FLT], [], 384, 1576, (0, 0, 2, 2), [1320, 1152, 984, 816]),
    12: ((10, 10, 6, 6), 1, [ICF], [], 448, 1640, (0, 0, 2, 2), [1384, 1216, 1048, 880]),
    13: ((11, 11, 11, 11), 1, [("z", "float", NAN)], [], 368, 1392, (0, 0, 1, 1), [800]),
    14: ((101, 101, 101, 101), 1, [("z", "icf", INT_MIN, 1000.0, 0.0, NAN)], ["LSOP12"], 392, 2344, (0, 0, 1, 1), [632]),
}


def sample_path(golden_dir, k):
    return os.path.join(golden_dir, "ref_samples", SAMPLES[k] + ".gvrs")


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) if isinstance(b, float) else a == b


def open_status(image):
    """gf_file_open on bytes: its status (the handle, if any, closed)"""
    image = np.frombuffer(bytes(image), np.uint8)
    h = _lib.C.c_void_p()
    buf = image.copy() if image.size else np.zeros(1, np.uint8)          # (an array of exactly the image's length)
    st = _lib.lib().gf_file_open(buf.ctypes.data, image.size, _lib.C.byref(h))
    assert (st == _lib.OK) == bool(h.value)
    _lib.lib().gf_file_close(h)
    return st


@pytest.mark.parametrize("k", range(15))
def test_samples_open_with_the_facts_of_the_reference(golden_dir, k):
    grid, checksums, elems, ids, content, directory, dir_rect, positions = FACTS[k]
    f = GvrsFileHip(sample_path(golden_dir, k))
    i = f.info
    assert (i["version"], i["subversion"]) == (1, 4) and i["checksum_enabled"] == checksums
    assert i["grid"] == grid and f.grid == grid
    assert i["elem_names"] == [e[0] for e in elems] and i["n_elems"] == len(elems)
    for got, spec, want in zip(i["elems"], f.elems, elems):
        kind = want[1]
        assert got["type"] == gridfour_amd.ELEM_TYPES[kind]
        if kind == "icf":
            assert spec[0] == "icf" and (got["fill_i"], got["scale"], got["offset"]) == (want[2], want[3], want[4]) and same(got["fill_f"], want[5])
        elif kind == "float":
            assert spec == "float" and same(got["fill_f"], want[2])
        else:
            assert spec == kind and got["fill_i"] == want[2]
    assert i["codec_ids"] == ids
    assert i["codecs"] == (STD_KINDS if ids == STD else [gridfour_amd.CODEC_LSOP12] if ids else [])
    assert (i["content_pos"], i["tile_dir_pos"], i["dir_entries_pos"]) == (content, directory, directory + 24)
    assert i["dir_extended"] == 0 and (i["dir_row0"], i["dir_col0"], i["dir_n_rows"], i["dir_n_cols"]) == dir_rect
    assert [f.tile_position(t) for t in range(len(positions))] == positions
    data = f.image.tobytes()
    for t, p in enumerate(positions):                         # a type-2 record whose tile-index word equals its slot
        assert data[p - 4] == 2 and struct.unpack_from("<i", data, p)[0] == t
    with pytest.raises(GvrsHipError):
        f.tile_position(len(positions))                      # outside the grid's tiles
    if k == 0:
        assert i["product_label"] == "Short, no nulls, not compressed"
    if k == 13:
        assert i["coordinate_system"] in (0, 1, 2) and i["metadata_dir_pos"] > 0 and i["freespace_dir_pos"] == 0
    f.close()


def sample01_facts():
    return dict(grid=(10, 10, 5, 5),
                elements=[B.element("zInt", "int", fill=INT_MIN, vmin=-20000, vmax=20000, label="Int", description="Integer", continuous=True)],
                tile_dir_pos=1384, metadata_dir_pos=1296, uuid=bytes.fromhex("f65831de71560c9eb149a7aadabae14e"),
                time_modified=0x184ae561011, product_label="Integer, no nulls, not compressed", size=368)


def test_builder_reproduces_the_header_of_sample01(golden_dir):
    data = open(sample_path(golden_dir, 1), "rb").read()
    facts = sample01_facts()
    head = B.header_record(**facts)
    assert len(head) == 384 and head == data[:384]


def small_file(**kw):
    """A 7 x 5 INT grid in 3 x 2 tiles, standard-form records of row * nCols + col, through the writer"""
    grid = kw.pop("grid", (7, 5, 3, 2))
    elements = kw.pop("elements", [B.element("z", "int")])
    cells = np.arange(grid[2] * grid[3], dtype=np.int32)
    n_tiles = -(-grid[0] // grid[2]) * -(-grid[1] // grid[3]) if kw.pop("with_records", True) else 0
    records = {t: B.standard_record(t, [cells + t]) for t in range(n_tiles)}
    return B.build_image(grid, elements, records, **kw)


def test_builder_images_open():
    image, positions = small_file(codec_ids=["GvrsHuffman", "MyOwnCodec", "LSOP08", "GvrsCanonicalHuffman"], extended=True, product_label="made here")
    f = GvrsFileHip(image)
    assert f.grid == (7, 5, 3, 2) and f.info["dir_extended"] == 1 and f.info["product_label"] == "made here"
    # an unknown codec id opens and is reported as such
    assert f.info["codecs"] == [gridfour_amd.CODEC_HUFFMAN, gridfour_amd.CODEC_UNKNOWN, gridfour_amd.CODEC_LSOP08, gridfour_amd.CODEC_CANON_HUFFMAN]
    assert f.info["codec_ids"][1] == "MyOwnCodec"
    assert [f.tile_position(t) for t in range(9)] == [positions[t] for t in range(9)]


REFUSALS = [
    ("magic", lambda im: b"Gvrs" + im[4:], _lib.ERR_FORMAT),
    ("version 1.05", lambda im: im[:13] + b"\x05" + im[14:], _lib.ERR_FORMAT),
    ("version 2.04", lambda im: im[:12] + b"\x02" + im[13:], _lib.ERR_FORMAT),
    ("version 1.01", lambda im: im[:13] + b"\x01" + im[14:], _lib.ERR_FORMAT),
    ("version 1.02", lambda im: im[:13] + b"\x02" + im[14:], _lib.ERR_UNSUPPORTED),
    ("version 1.03", lambda im: im[:13] + b"\x03" + im[14:], _lib.ERR_UNSUPPORTED),
    ("checksum", lambda im: im[:60] + bytes([im[60] ^ 1]) + im[61:], _lib.ERR_FORMAT),
    ("flag off, checksum left", lambda im: im[:128] + b"\0" + im[129:], _lib.ERR_FORMAT),
    ("empty", lambda im: b"", _lib.ERR_BOUNDS),
    ("head only", lambda im: im[:16], _lib.ERR_BOUNDS),
    ("inside the header record", lambda im: im[:200], _lib.ERR_BOUNDS),
    ("in front of the directory", lambda im: im[:struct.unpack_from("<q", im, 80)[0]], _lib.ERR_FORMAT),
    ("inside the directory's prefix", lambda im: im[:struct.unpack_from("<q", im, 80)[0] + 23], _lib.ERR_FORMAT),
]


@pytest.mark.parametrize("name,damage,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_on_a_damaged_image(name, damage, status):
    image, _ = small_file()
    assert open_status(image) == _lib.OK
    assert open_status(damage(image)) == status


FIELDS = [
    ("levels", dict(n_levels=2), _lib.ERR_FORMAT),
    ("opened for writing", dict(time_opened=1700000000000), _lib.ERR_FORMAT),
    ("type code 4", dict(type_codes=[4]), _lib.ERR_FORMAT),
    ("type code 255", dict(type_codes=[255]), _lib.ERR_FORMAT),
    ("no grid rows", dict(grid=(0, 5, 3, 2), with_records=False), _lib.ERR_FORMAT),
    ("no tile columns", dict(grid=(7, 5, 3, 0), with_records=False, dir_rect=(0, 0, 0, 0)), _lib.ERR_FORMAT),
    ("negative grid", dict(grid=(7, -5, 3, 2), with_records=False, dir_rect=(0, 0, 0, 0), domain=(0.0, 0.0, 1.0, 1.0)), _lib.ERR_FORMAT),
    ("17 elements", dict(elements=[B.element("e%d" % e, "short") for e in range(17)], with_records=False), _lib.ERR_UNSUPPORTED),
    ("256 codecs", dict(codec_ids=["c%d" % k for k in range(256)]), _lib.ERR_UNSUPPORTED),
    ("2^28 cells in a tile", dict(grid=(1 << 14, 1 << 14, 1 << 14, 1 << 14), with_records=False), _lib.ERR_UNSUPPORTED),
    ("2^32 tiles", dict(grid=(2 ** 31 - 1, 2, 1, 1), with_records=False, dir_rect=(0, 0, 0, 0)), _lib.ERR_UNSUPPORTED),
    ("16 elements, 255 codecs", dict(elements=[B.element("e%d" % e, "short") for e in range(16)], codec_ids=["c%d" % k for k in range(255)],
                                     with_records=False), _lib.OK),
]


@pytest.mark.parametrize("name,facts,status", FIELDS, ids=[r[0] for r in FIELDS])
def test_refusals_of_header_fields(name, facts, status):
    if facts.get("grid", (1, 1, 1, 1))[3] == 0:
        # (the writer divides by the tile size: lay the image out with a tile column and write the 0 afterwards)
        image, _ = small_file(**dict(facts, grid=(7, 5, 3, 2)))
        image = B.refresh_header_crc(image[:104 + 12] + struct.pack("<i", 0) + image[104 + 16:])
    else:
        image, _ = small_file(**facts)
    assert open_status(image) == status


def test_refusals_of_the_directory():
    image, _ = small_file()
    at = struct.unpack_from("<q", image, 80)[0]

    def with_dir_pos(p):
        return B.refresh_header_crc(image[:80] + struct.pack("<q", p) + image[88:])
    assert open_status(with_dir_pos(at)) == _lib.OK
    for p in (0, at + 4, 16, -8, len(image) - 16, len(image) + 800, 1 << 40):
        assert open_status(with_dir_pos(p)) == _lib.ERR_FORMAT, p
    for field, value in ((8, -1), (12, -1), (16, -3), (20, -1), (16, 1 << 20)):          # row0, col0, nRows, nCols of the rectangle
        bad = image[:at + field] + struct.pack("<i", value) + image[at + field + 4:]
        assert open_status(bad) == _lib.ERR_FORMAT, (field, value)
    # no columns means no entries: every tile is absent
    f = GvrsFileHip(image[:at + 20] + struct.pack("<i", 0) + image[at + 24:])
    assert (f.info["dir_n_rows"], f.info["dir_n_cols"]) == (0, 0) and [f.tile_position(t) for t in range(9)] == [0] * 9


def test_every_single_byte_change_of_the_header_region_is_refused(golden_dir):
    data = open(sample_path(golden_dir, 5), "rb").read()
    content = FACTS[5][4]
    rng = np.random.default_rng(5)
    for at in range(16, content):
        for x in (0x01, 0x80, 0xff, int(rng.integers(1, 256))):
            st = open_status(data[:at] + bytes([data[at] ^ x]) + data[at + 1:])
            assert st in (_lib.ERR_FORMAT, _lib.ERR_BOUNDS), (at, x, st)
    for at in (128,):                                        # the checksum flag itself, every other value
        for v in range(256):
            if v != data[at]:
                assert open_status(data[:at] + bytes([v]) + data[at + 1:]) in (_lib.ERR_FORMAT, _lib.ERR_BOUNDS), v


def test_every_prefix_of_sample14(golden_dir):
    data = open(sample_path(golden_dir, 14), "rb").read()
    enough = FACTS[14][5] + 24                               # the header record and the directory's prefix
    assert enough < len(data)
    for n in range(len(data) + 1):
        st = open_status(data[:n])
        assert (st == _lib.OK) == (n >= enough), n
        assert st in (_lib.OK, _lib.ERR_BOUNDS, _lib.ERR_FORMAT), (n, st)


def test_the_handle_keeps_nothing_of_the_image(golden_dir):
    data = open(sample_path(golden_dir, 6), "rb").read()
    L, h = _lib.lib(), _lib.C.c_void_p()
    buf = np.frombuffer(data, np.uint8).copy()
    assert L.gf_file_open(buf.ctypes.data, buf.size, _lib.C.byref(h)) == _lib.OK
    buf[:] = 0xee                                             # the bytes it was opened from are gone
    del buf
    info = np.zeros(1, gridfour_amd.codec._FILE_INFO)
    assert L.gf_file_get_info(h, info.ctypes.data) == _lib.OK and int(info[0]["content_pos"]) == FACTS[6][4]
    assert [L.gf_file_codec_id(h, k) for k in range(4)] == [b"GvrsHuffman", b"GvrsDeflate", b"GvrsFloat", None]
    assert L.gf_file_elem_name(h, 0) == b"zFlt" and L.gf_file_elem_name(h, 1) is None and L.gf_file_elem_name(h, -1) is None
    again = np.frombuffer(data, np.uint8).copy()             # the look-up takes the image anew
    pos = _lib.C.c_uint64()
    assert L.gf_file_tile_position(h, again.ctypes.data, again.size, 2, _lib.C.byref(pos)) == _lib.OK and pos.value == FACTS[6][7][2]
    L.gf_file_close(h)
    L.gf_file_close(None)
    assert L.gf_file_open(None, 10, _lib.C.byref(h)) == _lib.ERR_ARG and L.gf_file_get_info(None, None) == _lib.ERR_ARG


def test_damaged_directory_entries_on_the_host(golden_dir):
    """gf_file_tile_position judges an entry and the record head as the device form does (tests/test_gpu_file_read.py)"""
    for extended in (False, True):
        image, positions = small_file(extended=extended)
        f = GvrsFileHip(image)
        at, w = B.entry_offset(image, f.info, 4)
        pack = (lambda v: struct.pack("<q", v)) if extended else (lambda v: struct.pack("<I", (v // 8) & 0xffffffff))

        def status_with(entry_bytes, tile=4, im=image):
            bad = im[:at] + entry_bytes + im[at + w:]
            try:
                f.tile_position(tile, image=bad)
            except GvrsHipError as e:
                return e.status
            return _lib.OK
        assert status_with(pack(positions[4])) == _lib.OK
        assert status_with(pack(positions[5])) == _lib.ERR_FORMAT                     # another tile's record
        assert status_with(pack(f.info["content_pos"])) == _lib.ERR_BOUNDS             # in front of the first record's content
        assert status_with(pack(len(image) // 8 * 8)) == _lib.ERR_BOUNDS
        assert status_with(pack((len(image) - 8) // 8 * 8)) == _lib.ERR_BOUNDS         # within 12 bytes of the end
        if extended:
            assert status_with(pack(-8)) == _lib.ERR_BOUNDS
            assert status_with(pack(positions[4] + 4)) == _lib.ERR_BOUNDS
        else:
            assert status_with(struct.pack("<I", 0x80000000)) == _lib.ERR_BOUNDS
        assert f.tile_position(4, image=image[:at] + bytes(w) + image[at + w:]) == 0  # no such tile


@pytest.fixture(scope="module")
def parse_exe(tmp_path_factory):
    """(path, sanitized): the stand-alone program, with the address and undefined-behaviour sanitizers where their runtime is installed"""
    out = str(tmp_path_factory.mktemp("file_parse") / "file_parse_test")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
    tail = ["-o", out, os.path.join(HERE, "csrc", "file_parse_test.cpp")]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + tail, capture_output=True, text=True)
    if r.returncode == 0:
        return out, True
    subprocess.check_call(base + tail)
    return out, False


def test_parser_alone_under_the_sanitizers(parse_exe, golden_dir):
    exe, sanitized = parse_exe
    paths = [sample_path(golden_dir, k) for k in range(15)]
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 16 and lines[-1].startswith("done")
    for k, line in enumerate(lines[:15]):
        grid, checksums, elems, ids, content, directory, _, positions = FACTS[k]
        want = "%s 1.04 grid %d %d %d %d checksums %d elems %d codecs %d content %d dir %d tiles %s" % (
            (paths[k],) + grid + (checksums, len(elems), len(ids), content, directory, " ".join(str(p) for p in positions)))
        assert line == want
    if not sanitized:
        pytest.skip("the sanitizer runtime is not installed: the program was built plain and has passed")
