"""gf_file_assemble and gf_file_write_plan without a GPU: the reference's fifteen sample files taken apart and assembled again,
byte for byte; the emitters alone under the sanitizers (tests/csrc/file_emit_test.cpp); every image the emitter writes opened by
gf_file_open with the facts that went in; the Python reference writer of gvrs_file_write_ref.py against the assembler; refusals."""
import os
import struct
import subprocess

import numpy as np
import pytest

import gridfour_amd
from gridfour_amd import GvrsFileFacts, GvrsFileHip, GvrsHipError, FILE_DIR_EXTENDED
from gridfour_amd import _lib

import gvrs_file_build as B
import gvrs_file_write_ref as W
from test_file_open import SAMPLES, sample_path

HERE = os.path.dirname(os.path.abspath(__file__))
INT_MIN = -2 ** 31


@pytest.mark.parametrize("k", range(15))
def test_samples_are_reproduced_byte_for_byte(golden_dir, k):
    """Facts, metadata records' fields and tile records (in file order: 3, 2, 1, 0 where there are four) from the file; the image
    must equal the file: header, metadata, both directories, padding and every CRC are then the reference's."""
    s, records, data = W.sample_spec(sample_path(golden_dir, k))
    if len(records) == 4:
        assert [t for t, _ in records] == [3, 2, 1, 0]
    image = GvrsFileHip.assemble(W.lib_facts(s), [r for _, r in records], [t for t, _ in records])
    assert len(image) == len(data)
    assert image == data
    if SAMPLES[k] == "Sample08_MixedTypes":                   # checksums off: every CRC word is 0
        assert not s["checksums"] and all(struct.unpack_from("<I", rec, len(rec) - 4)[0] == 0 for _, rec in records)
        (size,) = struct.unpack_from("<i", image, 16)
        assert struct.unpack_from("<I", image, 16 + size - 4)[0] == 0 and struct.unpack_from("<I", image, len(image) - 4)[0] == 0


def build_emit_test(tmp_path_factory, sanitized):
    out = str(tmp_path_factory.mktemp("file_emit") / ("file_emit_test" + ("_san" if sanitized else "")))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
    cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitized else []
    r = subprocess.run(cmd + ["-o", out, os.path.join(HERE, "csrc", "file_emit_test.cpp")], capture_output=True, text=True)
    return out if r.returncode == 0 else None, r.stderr


@pytest.fixture(scope="module")
def emit_exe(tmp_path_factory):
    out, err = build_emit_test(tmp_path_factory, False)
    assert out, err[-4000:]
    return out


def run_emit_test(exe, golden_dir):
    paths = [sample_path(golden_dir, k) for k in range(15)]
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 17 and lines[0].startswith("chunk ") and lines[-1] == "done"
    for k, line in enumerate(lines[1:16]):
        assert line.startswith("%s same %d records " % (paths[k], os.path.getsize(paths[k]))), line


def test_emitters_alone(emit_exe, golden_dir):
    """The fifteen reproductions, every image_cap from 0 to the need for two of them (below the need: GF_ERR_CAPACITY and no write,
    checked with a guard region), the empty and the forced extended directory, metadata of length 0, the CRC fold for every pair
    of lengths 0 .. 2 chunks + 1."""
    run_emit_test(emit_exe, golden_dir)


def test_emitters_alone_under_the_sanitizers(tmp_path_factory, golden_dir):
    out, err = build_emit_test(tmp_path_factory, True)
    if out is None:
        pytest.skip("the sanitizer runtime is not installed: the plain program runs in test_emitters_alone")
    run_emit_test(out, golden_dir)


def crc_chunk(exe):
    """GF_FILE_CRC_CHUNK as the stand-alone program prints it (tests/test_gpu_file_write.py takes it from here)"""
    line = subprocess.run([exe], capture_output=True, text=True).stdout.splitlines()[0]
    assert line.startswith("chunk ")
    return int(line.split()[1])


def test_chunk_size_is_printed(emit_exe):
    c = crc_chunk(emit_exe)
    assert c >= 64 and c % 64 == 0


@pytest.mark.parametrize("extended", [False, True], ids=["compact", "extended"])
def test_directory_of_more_than_64_chunks(emit_exe, extended):
    """The shape at which the device's fold gives a lane a second chunk (tests/dir_seams.py), on the host: the assembler's chunked
    fold against the Python writer and against a Python CRC loop that is not the library's"""
    import gvrs_file_update_ref as R
    from dir_seams import SEAMS
    w = 8 if extended else 4
    n = dict(SEAMS)["65C+1"](crc_chunk(emit_exe), w)
    s = W.spec((2, 2 * n, 2, 2), [B.element("z_int", "int")], [], uuid=bytes(16), time_modified=5)
    recs = [B.frame_record(t, [struct.pack("<4i", t, t + 1, t + 2, t + 3)], True) for t in range(n)]
    flags = FILE_DIR_EXTENDED if extended else 0
    image = GvrsFileHip.assemble(W.lib_facts(s), recs, np.arange(n, dtype=np.int32), flags=flags)
    assert image == W.ref_image(s, list(enumerate(recs)), extended=extended)
    at = GvrsFileHip(image).info["tile_dir_pos"] - 8
    (size,) = struct.unpack_from("<i", image, at)
    assert at + size == len(image) and size == (8 + 8 + 16 + n * w + 4 + 7) // 8 * 8 and size - 4 > 64 * crc_chunk(emit_exe)
    assert struct.unpack_from("<I", image, at + size - 4)[0] == R.crc32c(image[at:at + size - 4])


def test_exported_crc32c_against_a_bit_by_bit_loop():
    """gf_crc32c through the binding, as tests/csrc/file_emit_test.cpp holds the library's own gfCrc32c: every length 0 .. 40 at
    every start offset 0 .. 7 of a buffer (head, 8-byte body and tail of an eight-byte step), and the check value"""
    def bitwise(data):
        crc = 0xffffffff
        for x in data:
            crc ^= x
            for _ in range(8):
                crc = (crc >> 1) ^ (0x82F63B78 if crc & 1 else 0)
        return crc ^ 0xffffffff

    buf = np.random.default_rng(40).integers(0, 256, 48, dtype=np.uint8).tobytes()
    assert bitwise(b"123456789") == 0xE3069283 and B.crc32c(b"123456789") == 0xE3069283
    for at in range(8):
        for n in range(41):
            assert B.crc32c(buf[at:at + n]) == bitwise(buf[at:at + n]), (at, n)


def random_spec(rng, n_elems):
    kinds = ["int", "short", "float", "icf"]
    elements = []
    for e in range(n_elems):
        kind = kinds[e % 4] if e < 4 else kinds[int(rng.integers(4))]
        name = "el%d_%s" % (e, "x" * int(rng.integers(0, 6)))
        text = dict(label="L" * int(rng.integers(0, 5)), description="d" * int(rng.integers(0, 9)), unit="u" * int(rng.integers(0, 3)),
                    continuous=bool(rng.integers(2)))
        if kind == "int":
            elements.append(B.element(name, kind, fill=int(rng.integers(-99, 99)), vmin=-1000, vmax=int(rng.integers(1000, 5000)), **text))
        elif kind == "short":
            elements.append(B.element(name, kind, fill=int(rng.integers(-99, 99)), vmin=-500, vmax=500, **text))
        elif kind == "float":
            elements.append(B.element(name, kind, fill=float(rng.integers(-9, 9)), vmin=-1.5, vmax=2.5e6, **text))
        else:
            elements.append(B.element(name, kind, fill=int(rng.integers(-99, 99)), vmin=INT_MIN + 1, vmax=2 ** 31 - 2,
                                      scale=float(2.0 ** int(rng.integers(-2, 5))), offset=float(rng.integers(-3, 4)),
                                      fill_f=float(rng.integers(-9, 9)), **text))
    return elements


@pytest.mark.parametrize("n_elems", [1, 2, 3, 4, 5, 9, 16])
def test_emitted_images_open_with_the_facts_that_went_in(n_elems):
    rng = np.random.default_rng(100 + n_elems)
    ids = [["GvrsHuffman", "GvrsDeflate", "GvrsFloat"], [], ["LSOP08", "GvrsCanonicalHuffman"]][n_elems % 3]
    grid = (int(rng.integers(5, 40)), int(rng.integers(5, 40)), int(rng.integers(1, 7)), int(rng.integers(1, 7)))
    metadata = [("m%d" % k, k, k % 7, bytes(rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8)), "about %d" % k) for k in range(n_elems % 4)]
    s = W.spec(grid, random_spec(rng, n_elems), ids, checksums=bool(n_elems % 2), metadata=metadata, uuid=bytes(rng.integers(0, 256, 16, dtype=np.uint8)),
               time_modified=int(rng.integers(1, 1 << 40)), raster_space=n_elems % 2, coordinate_system=n_elems % 3, domain=(-3.5, 2.25, 100.0, 77.5),
               cell_size=(0.5, 0.25), m2r=(2.0, 0.0, 7.0, 0.0, 4.0, -9.0), r2m=(0.5, 0.0, -3.5, 0.0, 0.25, 2.25), product_label="p" * n_elems)
    n_tile_cols = -(-grid[1] // grid[3])
    n_tiles = -(-grid[0] // grid[2]) * n_tile_cols
    tiles = sorted(rng.choice(n_tiles, size=min(n_tiles, 5), replace=False).tolist(), reverse=True)
    cells = grid[2] * grid[3]
    dtype = {"int": np.int32, "short": np.int16, "float": np.float32, "icf": np.int32}
    records = [(t, B.standard_record(t, [np.full(cells, t, dtype[el["kind"]]) for el in s["elements"]], s["checksums"])) for t in tiles]
    for flags in (0, FILE_DIR_EXTENDED):
        image = GvrsFileHip.assemble(W.lib_facts(s), [r for _, r in records], [t for t, _ in records], flags=flags)
        assert image == W.ref_image(s, records, extended=bool(flags))
        f = GvrsFileHip(image)
        i = f.info
        assert f.grid == grid and i["n_elems"] == n_elems and i["checksum_enabled"] == int(s["checksums"])
        assert i["elem_names"] == [el["name"] for el in s["elements"]] and i["codec_ids"] == ids and i["codecs"] == [W.KINDS[c] for c in ids]
        assert (i["raster_space"], i["coordinate_system"], i["product_label"]) == (n_elems % 2, n_elems % 3, "p" * n_elems)
        assert (i["x0"], i["y0"], i["x1"], i["y1"], i["cell_size_x"], i["cell_size_y"]) == (-3.5, 2.25, 100.0, 77.5, 0.5, 0.25)
        assert tuple(i["m2r"]) == (2.0, 0.0, 7.0, 0.0, 4.0, -9.0) and tuple(i["r2m"]) == (0.5, 0.0, -3.5, 0.0, 0.25, 2.25)
        assert i["dir_extended"] == int(bool(flags)) and i["freespace_dir_pos"] == 0 and (i["metadata_dir_pos"] != 0) == bool(metadata)
        for got, el in zip(i["elems"], s["elements"]):
            assert got["type"] == gridfour_amd.ELEM_TYPES[el["kind"]]
            if el["kind"] == "icf":
                assert (got["fill_i"], got["scale"], got["offset"], got["fill_f"]) == (el["fill"], el["scale"], el["offset"], el["fill_f"])
            elif el["kind"] == "float":
                assert got["fill_f"] == el["fill"]
            else:
                assert got["fill_i"] == el["fill"]
        rows, cols = [t // n_tile_cols for t in tiles], [t % n_tile_cols for t in tiles]
        assert (i["dir_row0"], i["dir_col0"], i["dir_n_rows"], i["dir_n_cols"]) == (min(rows), min(cols), max(rows) - min(rows) + 1,
                                                                                     max(cols) - min(cols) + 1)
        first, most = W.lib_facts(s).plan()
        at = first
        for t, rec in records:                                # the caller's order, end to end behind the metadata records
            assert f.tile_position(t) == at + 8
            at += len(rec)
        assert [f.tile_position(t) for t in range(n_tiles) if t not in tiles] == [0] * (n_tiles - len(tiles))
        assert len(image) <= most
        f.close()


def small():
    s = W.spec((7, 5, 3, 2), [B.element("z", "int")], ["GvrsHuffman"], metadata=[("n", 1, 2, b"abc", "d")])
    cells = np.arange(6, dtype=np.int32)
    return s, [(t, B.standard_record(t, [cells + t])) for t in (4, 0, 7)]


def test_records_of_length_zero_and_the_empty_directory():
    s, records = small()
    with_empty = [records[0], (2, b""), records[1], (8, b""), records[2]]
    image = GvrsFileHip.assemble(W.lib_facts(s), [r for _, r in with_empty], [t for t, _ in with_empty])
    assert image == W.ref_image(s, records) == W.ref_image(s, with_empty)
    none = GvrsFileHip.assemble(W.lib_facts(s), [b"", b""], [1, 5])
    assert none == W.ref_image(s, []) and none == GvrsFileHip.assemble(W.lib_facts(s), [], [])
    f = GvrsFileHip(none)
    assert (f.info["dir_row0"], f.info["dir_col0"], f.info["dir_n_rows"], f.info["dir_n_cols"]) == (0, 0, 0, 0)
    assert len(none) == f.info["tile_dir_pos"] - 8 + 40 and struct.unpack_from("<i", none, f.info["tile_dir_pos"] - 8)[0] == 40


def test_capacity_and_refusals():
    s, records = small()
    facts, recs, idx = W.lib_facts(s), [r for _, r in records], [t for t, _ in records]
    whole = GvrsFileHip.assemble(facts, recs, idx)
    for cap in (0, 16, len(whole) - 8, len(whole) - 1):
        st, image, need = GvrsFileHip.assemble(facts, recs, idx, image_cap=cap, return_code=True)
        assert st == _lib.ERR_CAPACITY and need == len(whole) and image == b"\xa5" * cap
    st, image, need = GvrsFileHip.assemble(facts, recs, idx, image_cap=len(whole), return_code=True)
    assert st == _lib.OK and image == whole

    def status(recs=recs, idx=idx, facts=facts):
        return GvrsFileHip.assemble(facts, recs, idx, image_cap=4096, return_code=True)[0]
    assert status(idx=[4, 0, 4]) == _lib.ERR_ARG                             # two non-empty records of one tile
    assert status(recs=[recs[0], b"", recs[2]], idx=[4, 4, 7]) == _lib.OK    # ... an empty one beside it is none
    assert status(idx=[4, 0, 9]) == _lib.ERR_ARG and status(idx=[4, -1, 7]) == _lib.ERR_ARG      # outside the grid's 9 tiles
    assert status(recs=[recs[0], b"", recs[2]], idx=[4, 9, 7]) == _lib.ERR_ARG
    assert status(recs=[recs[0][:-4], recs[1], recs[2]]) == _lib.ERR_ARG    # no multiple of 8
    assert status(facts=W.lib_facts(dict(s, codec_ids=["MyOwnCodec"]))) == _lib.ERR_UNSUPPORTED
    assert status(facts=GvrsFileFacts((7, 5, 3, 0), ["int"])) == _lib.ERR_ARG
    with pytest.raises(GvrsHipError):
        GvrsFileFacts((7, 5, 3, 2), ["int"] * 17).plan()
    L = _lib.lib()
    need = _lib.C.c_uint64()
    assert L.gf_file_assemble(None, None, 0, 0, None, None, None, 0, None, 0, _lib.C.byref(need)) == _lib.ERR_ARG
    assert L.gf_file_assemble(*facts.args(), 0, None, None, None, 0, None, 0, None) == _lib.ERR_ARG


def test_plan_bounds_every_rectangle():
    s, _ = small()
    facts = W.lib_facts(s)
    first, most = facts.plan()
    assert first % 8 == 0 and first == len(W.ref_image(s, [])) - 40 - len(W.frame(4, b"\0" * (4 + 8 + 3 + 4 + 1), True))
    record = int(_lib.lib().gf_tile_record_max_bytes_elems(facts.specs.ctypes.data, 1, 3, 2))
    meta_dir = len(W.frame(4, b"\0" * (4 + 8 + 3 + 4 + 1), True))
    assert most == first + 9 * record + meta_dir + (8 + 8 + 16 + 9 * 4 + 4 + 7) // 8 * 8
    assert facts.plan(rect=(3, 2, 1, 1))[1] == first + record + meta_dir + 40
    assert facts.plan(flags=FILE_DIR_EXTENDED)[1] == first + 9 * record + meta_dir + (8 + 8 + 16 + 9 * 8 + 4 + 7) // 8 * 8
