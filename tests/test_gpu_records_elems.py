"""Tile records of several elements and of float / int-coded-float elements (gf_tile_record_decode_batch_elems_dev and its host
form): the reference's own sample files; one element, and gf_tile_record_decode_batch_dev beside it, against the host call
gf_tile_record_decode_batch; three elements framed here from the existing encoders' packings against the existing host decoders;
the ICF arithmetic bit for bit against numpy float32; damaged records; the host form against the device form."""
import itertools
import os
import struct

import numpy as np
import pytest

import damage as D
from gvrs_walk import walk_records
from test_gpu_records_dev import LIST5, NC, NR, _concat, _crc, _flip, _frame_elems, _host_records, _put32, _refresh_crc, _shifted
from test_gpu_records_dev import ctx, master5, mixed_int, mixed_short      # noqa: F401  (fixtures)
from tilegen import make_tile

pytestmark = pytest.mark.gpu
NULL = -2**31
NAN = np.float32(np.nan)
ICF3 = ("icf", 100.0, -5.25, -9999, NAN)
ELEMS3 = ["short", ICF3, "float"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _icf_expect(codes, el):
    """TileElementIntCodedFloat.getValue in numpy float32: one rounding per step"""
    _, scale, offset, fill_i, fill_f = el
    codes = np.asarray(codes, np.int32)
    with np.errstate(all="ignore"):
        v = codes.astype(np.float32) / np.float32(scale) + np.float32(offset)
    return np.where(codes == np.int32(fill_i), np.float32(fill_f), v).astype(np.float32)


# ---------------------------------------------------------------- 1. the reference's own bytes

def _ramp_fill(idx, grid, tile, fill, dtype):
    """tile idx of a grid x grid raster cut into tile x tile tiles: row * grid + col - 1 on the grid, fill outside it"""
    per_row = -(-grid // tile)
    tr, tc = divmod(idx, per_row)
    rows = np.arange(tile)[:, None] + tr * tile
    cols = np.arange(tile)[None, :] + tc * tile
    v = (rows * grid + cols - 1).astype(dtype)
    return np.where((rows < grid) & (cols < grid), v, np.asarray(fill, dtype)).astype(dtype).ravel()


ICF1 = ("icf", 1.0, 0.0, NULL, NAN)
SAMPLES = [
    # file, codec list (None: the standard list), tile size, grid size, elements, verify checksums, fills of the expected ramp
    ("Sample02_FltNoComp.gvrs", [], 5, 10, ["float"], True, [NAN]),
    ("Sample11_FltNoComp.gvrs", [], 6, 10, ["float"], True, [NAN]),
    ("Sample06_FltComp.gvrs", None, 50, 100, ["float"], True, [NAN]),
    ("Sample03_ICFNoComp.gvrs", [], 5, 10, [ICF1], True, [NAN]),
    ("Sample12_ICFNoComp.gvrs", [], 6, 10, [ICF1], True, [NAN]),
    ("Sample07_ICFComp.gvrs", None, 50, 100, [ICF1], True, [NAN]),
    ("Sample08_MixedTypes.gvrs", [], 5, 10, ["short", "float"], False, [-32768, NAN]),      # (the file's CRC words are zero)
    ("Sample09_ShortNoComp.gvrs", [], 6, 10, ["short"], True, [-32768]),
    ("Sample10_IntNoComp.gvrs", [], 6, 10, ["int"], True, [NULL]),
]


def _sample_blob(golden_dir, name):
    """the tile records of a sample file as they lie in it (with whatever lies between them): (blob, offsets, tile indices, contents)"""
    with open(os.path.join(golden_dir, "ref_samples", name), "rb") as f:
        data = f.read()
    spans = sorted((pos, size, struct.unpack_from("<i", content, 0)[0], content) for pos, size, rtype, content in walk_records(data) if rtype == 2)
    lo = spans[0][0] & ~3
    hi = spans[-1][0] + spans[-1][1]
    offsets = np.array([p - lo for p, _, _, _ in spans] + [hi - lo], np.uint64)
    return np.frombuffer(data[lo:hi], np.uint8), offsets, [i for _, _, i, _ in spans], [c for _, _, _, c in spans]


def _np_dtype(el):
    return {"int": np.int32, "short": np.int16}.get(el if isinstance(el, str) else el[0], np.float32)


@pytest.mark.parametrize("name,codecs,tile,grid,elems,verify,fills", SAMPLES, ids=[c[0][:8] for c in SAMPLES])
def test_reference_sample_records(golden_dir, ctx, name, codecs, tile, grid, elems, verify, fills):
    import gridfour_amd
    master = gridfour_amd.CodecMasterHip(context=ctx) if codecs is None else gridfour_amd.CodecMasterHip(codec_list=codecs, context=ctx)
    blob, offsets, want_idx, contents = _sample_blob(golden_dir, name)
    assert len(want_idx) == 4
    if name.startswith("Sample08"):
        assert all(struct.unpack_from("<i", c, 4)[0] == 52 and struct.unpack_from("<i", c, 60)[0] == 100 for c in contents)   # byte 68 of the record
    idx, vals, st = master.record_blob_elems_dev(tile, tile, blob, offsets, elems, verify_checksums=verify)
    assert st.shape == (len(elems), 4) and (st == 0).all(), st
    assert list(idx) == want_idx
    for e, el in enumerate(elems):
        dt = _np_dtype(el)
        want = np.stack([_ramp_fill(i, grid, tile, fills[e], dt) for i in want_idx])
        assert vals[e].dtype == dt
        if dt == np.float32:
            assert np.array_equal(_bits(vals[e]), _bits(want)), (name, e)                 # (NaN outside the grid: bit patterns)
        else:
            assert np.array_equal(vals[e], want), (name, e)
    if len(elems) == 1 and elems[0] in ("int", "short"):                                  # the same as the old call
        oi, ov, os_ = master.record_blob_dev(tile, tile, blob, offsets, element=elems[0], verify_checksums=verify)
        assert np.array_equal(os_, st[0]) and np.array_equal(oi, idx) and np.array_equal(ov, vals[0])


def test_reference_sample_model_coordinates(golden_dir, ctx):
    """Sample13: one 11 x 11 float tile in standard form -- the cells are the file's bytes"""
    import gridfour_amd
    master = gridfour_amd.CodecMasterHip(context=ctx)
    blob, offsets, want_idx, contents = _sample_blob(golden_dir, "Sample13_ModelCoord.gvrs")
    assert want_idx == [0] and struct.unpack_from("<i", contents[0], 4)[0] == 484
    idx, vals, st = master.record_blob_elems_dev(11, 11, blob, offsets, ["float"], verify_checksums=True)
    assert (st == 0).all() and list(idx) == [0]
    assert np.array_equal(_bits(vals[0][0]), np.frombuffer(contents[0][8:8 + 484], "<u4"))
    assert np.isfinite(vals[0]).all() and abs(float(vals[0].max()) - 1.0) < 1e-6           # z = sin(x pi) sin(y pi) on [0, 1]^2


# ---------------------------------------------------------------- 2. one element: both device calls equal the host call

@pytest.fixture(scope="module")
def damaged_packings():
    """packings of one 40 x 60 tile damaged by tests/damage.py (a spread of its kinds), for the two Huffman codecs of LIST5"""
    import oracle
    values = make_tile("smooth", NR, NC, seed=31).astype(np.int32)
    out = []
    for kind, slot, enc in ((D.HUFFMAN, 0, oracle.codec_huffman_encode), (D.CANON, 3, oracle.codec_canon_encode)):
        pk = enc(slot, NR, NC, values)
        pk = pk[0] if isinstance(pk, tuple) else pk
        kept = [p for _, p in D.damage_set(pk, kind, NR, NC, seed=17) if D.deviation(p, kind, NR * NC) is None and len(p) not in (NR * NC * 4, NR * NC * 2)]
        out += kept[::max(1, len(kept) // 12)]
    assert len(out) >= 20
    return out


@pytest.mark.parametrize("element", ["int", "short"])
def test_one_element_equals_the_old_call(master5, mixed_int, mixed_short, damaged_packings, element):
    records, elements, tiles = mixed_int if element == "int" else mixed_short
    std = NR * NC * (2 if element == "short" else 4)
    assert sum(len(el) == std for el in elements) >= 3 and sum(len(el) != std for el in elements) >= 12
    r = next(rec for rec, el in zip(records, elements) if len(el) != std)
    framing = [_refresh_crc(r[:4] + b"\x03" + r[5:]), _put32(r, 0, len(r) + 4), _put32(r, 0, 16), _refresh_crc(_put32(r, 12, len(r) - 15)),
               _refresh_crc(r[:16] + b"\x05" + r[17:]), _refresh_crc(r[:16] + b"\x02" + r[17:]), _refresh_crc(_put32(r, 12, 0)),
               _flip(r, 9, 2), _flip(r, 16 + 7, 5), r[:12]]
    bad = [_frame_elems(5000 + i, [p]) for i, p in enumerate(damaged_packings)] + framing
    batch = list(records)
    for i, rec in enumerate(bad):                                  # damaged records spread among the good ones
        batch.insert((3 * i + 1) % len(batch), rec)
    blob, offsets = _shifted(batch, seed=3)
    assert {int(o) % 2 for o in offsets[:-1]} == {0, 1}
    for verify in (True, False):
        hi, hv, hs = _host_records(master5, NR, NC, blob, offsets, element, verify)      # (gf_tile_record_decode_batch: its own code)
        oi, ov, os_ = master5.record_blob_dev(NR, NC, blob, offsets, element=element, verify_checksums=verify)
        ni, nv, ns = master5.record_blob_elems_dev(NR, NC, blob, offsets, [element], verify_checksums=verify)
        assert ns.shape == (1, len(batch))
        ok = hs == 0
        for what, di, dv, ds in (("the record call", oi, ov, os_), ("the elements call", ni, nv[0], ns[0])):
            assert np.array_equal(ds, hs), (what, verify, ds.tolist(), hs.tolist())
            assert np.array_equal(di, hi), (what, verify)
            assert dv.dtype == hv.dtype and np.array_equal(dv[ok], hv[ok]), (what, verify)
        assert ok.sum() >= len(records) and (hs == -1).sum() >= 5 and (hs == -2).sum() >= 3


# ---------------------------------------------------------------- 3. three elements

N3 = 70
SHAPES3 = [(5, 5), (7, 9), (40, 60)]


def _three_sources(nr, nc):
    """per record: short cells (as ints for the codecs, with nulls), ICF codes (with the fill code), floats (with specials)"""
    cells = nr * nc
    kinds = ["smooth", "noise8", "steps", "ramp", "noise16"]
    rng = np.random.default_rng(cells)
    s = np.stack([np.clip(make_tile(kinds[i % 5], nr, nc, seed=200 + i), -32767, 32767) for i in range(N3)]).astype(np.int32)
    c = np.stack([make_tile(kinds[(i + 2) % 5], nr, nc, seed=300 + i) for i in range(N3)]).astype(np.int32)
    c[c == NULL] = 7
    f = (np.stack([make_tile("smooth", nr, nc, seed=400 + i) for i in range(N3)]).astype(np.float32) * np.float32(0.37)).astype(np.float32)
    for i in range(N3):
        s[i, rng.integers(0, cells, 3)] = NULL
        c[i, rng.integers(0, cells, 3)] = -9999
        f[i, rng.integers(0, cells, 4)] = np.array([np.nan, -0.0, np.inf, 1e-42], np.float32)
    return s, c, f


@pytest.fixture(scope="module")
def three(ctx):
    """per shape: the blob and offsets of 70 three-element records, what they hold, and the device form's answer (shared by tests 3 and 6)"""
    import gridfour_amd
    master = gridfour_amd.CodecMasterHip(codec_list=LIST5, context=ctx)
    enc = gridfour_amd.CodecMasterHip(context=ctx)                      # the standard list: LIST5's entries 0 .. 3
    flt = gridfour_amd.CodecFloatHip(context=ctx, level=6)
    out = {}
    for nr, nc in SHAPES3:
        cells = nr * nc
        src = _three_sources(nr, nc)
        std_size = [(2 * cells + 3) & ~3, 4 * cells, 4 * cells]
        packs = [enc.encode_batch(nr, nc, src[0])[0], enc.encode_batch(nr, nc, src[1])[0], flt.encode_floats_batch(2, nr, nc, src[2])]
        std = [np.where(src[0] == NULL, -32768, src[0]).astype("<i2"), src[1].astype("<i4"), src[2].astype("<f4")]
        elements = []                                                  # [record][element] bytes
        for i in range(N3):
            els = []
            for e in range(3):
                if (i >> e) & 1:                                       # every combination packed / standard over i mod 8
                    pk = packs[e][i]
                    assert pk is not None
                    pk += b"\0" * ((i // 8 + e * (i // 16) - len(pk)) % 4)     # (trailing bytes no decoder looks at: its length mod 4
                                                                               # is chosen, and with it the next element's residue)
                    if len(pk) == std_size[e]:
                        pk += b"\0\0\0\0"
                    els.append(pk)
                else:
                    els.append(std[e][i].tobytes() + b"\0" * (std_size[e] - std[e][i].nbytes))
            elements.append(els)
        records = [_frame_elems(100 + 3 * i, els) for i, els in enumerate(elements)]
        blob, offsets = _shifted(records, seed=cells)
        got = master.record_blob_elems_dev(nr, nc, blob, offsets, ELEMS3, verify_checksums=True)
        out[(nr, nc)] = dict(master=master, flt=flt, src=src, std_size=std_size, elements=elements, blob=blob, offsets=offsets, got=got)
    return out


@pytest.mark.parametrize("nr,nc", SHAPES3)
def test_three_elements(three, nr, nc):
    t = three[(nr, nc)]
    cells, elements, offsets, std_size = nr * nc, t["elements"], t["offsets"], t["std_size"]
    idx, vals, st = t["got"]
    assert st.shape == (3, N3) and list(idx) == [100 + 3 * i for i in range(N3)]
    # what the batch covers: blob offsets of both parities; later elements (and ICF elements in standard form) at every residue
    assert {int(o) % 2 for o in offsets[:-1]} == {0, 1}
    for e in (1, 2):
        starts = [16 + sum(4 + len(x) for x in els[:e]) for els in elements]
        assert {s % 4 for s in starts} == {0, 1, 2, 3}, (e, "relative to the record")
    icf_std = {(int(offsets[i]) + 20 + len(els[0])) % 4 for i, els in enumerate(elements) if len(els[1]) == std_size[1]}
    assert icf_std == {0, 1, 2, 3}
    assert {tuple(len(x) == n for x, n in zip(els, std_size)) for els in elements} == set(itertools.product((False, True), repeat=3))
    # expected: the existing host decoders on the same element bytes, then the element's own conversion
    want, want_st = [], []
    for e in range(3):
        packed = [i for i, els in enumerate(elements) if len(els[e]) != std_size[e]]
        pk = [elements[i][e] for i in packed]
        dec, dst = t["flt"].decode_floats_batch(nr, nc, pk) if e == 2 else t["master"].decode_batch(nr, nc, pk)
        assert (dst == 0).all()
        full = np.zeros((N3, cells), np.float32 if e == 2 else np.int32)
        full[:] = t["src"][e]                                            # (standard form: the cells themselves)
        full[packed] = dec
        assert np.array_equal(full.view(np.uint32), t["src"][e].view(np.uint32))      # the codecs are lossless
        want.append(full)
        want_st.append(np.zeros(N3, np.int32))
    assert np.array_equal(st, np.stack(want_st)), st.tolist()
    assert vals[0].dtype == np.int16 and np.array_equal(vals[0], np.where(want[0] == NULL, -32768, want[0]).astype(np.int16))
    assert vals[1].dtype == np.float32 and np.array_equal(_bits(vals[1]), _bits(_icf_expect(want[1], ICF3)))
    assert np.isnan(vals[1]).sum() == (want[1] == -9999).sum() > 0
    assert vals[2].dtype == np.float32 and np.array_equal(_bits(vals[2]), _bits(want[2]))


# ---------------------------------------------------------------- 4. ICF numeric edges

def test_icf_numeric_edges(ctx):
    """a 4 x 4 tile of edge codes, in standard form and packed, under twelve (scale, offset) pairs at once: twelve ICF elements"""
    import gridfour_amd
    master = gridfour_amd.CodecMasterHip(codec_list=LIST5, context=ctx)
    codes = np.array([0, 1, -1, 2**24 + 1, 2**31 - 1, -2**31 + 1, -9999, NULL, -(2**24 + 1), 2**24 + 3, 123456789, -987654321,
                      9999, 3, 1000, -2**31 + 2], np.int32)
    pk = master.encode_batch(4, 4, codes[None])[0][0]
    assert pk is not None and len(pk) != 64
    elems = [("icf", np.float32(s), np.float32(o), NULL if k % 2 else -9999, NAN if k % 3 else np.float32(-1.0))
             for k, (s, o) in enumerate(itertools.product((1.0, 3.0, np.float32(0.1), np.float32(1e-3)), (0.0, -5.25, 1e7)))]
    assert len(elems) == 12
    records = [_frame_elems(0, [codes.astype("<i4").tobytes()] * 12), _frame_elems(1, [pk] * 12),
               _frame_elems(2, [pk if e % 2 else codes.astype("<i4").tobytes() for e in range(12)])]
    for blob, offsets in (_concat(records), _shifted(records, seed=9)):
        idx, vals, st = master.record_blob_elems_dev(4, 4, blob, offsets, elems, verify_checksums=True)
        assert (st == 0).all() and list(idx) == [0, 1, 2]
        for e, el in enumerate(elems):
            want = _icf_expect(codes, el)
            assert np.isnan(want).any() or (want == -1.0).any()
            for t in range(3):
                assert np.array_equal(_bits(vals[e][t]), _bits(want)), (e, t, el, vals[e][t].tolist(), want.tolist())


# ---------------------------------------------------------------- 5. damage

ELEMS5 = ["int", ICF3, "float"]
R5, C5 = 7, 9


@pytest.fixture(scope="module")
def damage5(ctx):
    """twelve good all-packed records of [INT, ICF, FLOAT] and the damaged forms of six of them: (master, good, bad, cells per element)"""
    import gridfour_amd
    master = gridfour_amd.CodecMasterHip(codec_list=LIST5, context=ctx)
    enc = gridfour_amd.CodecMasterHip(context=ctx)                      # the standard list: LIST5's entries 0 .. 3
    flt = gridfour_amd.CodecFloatHip(context=ctx, level=6)
    s, c, f = _three_sources(R5, C5)
    s, c, f = s[:12], c[:12], f[:12]
    packs = [enc.encode_batch(R5, C5, s)[0], enc.encode_batch(R5, C5, c)[0], flt.encode_floats_batch(2, R5, C5, f)]
    std = 4 * R5 * C5
    assert all(p is not None and len(p) != std for e in range(3) for p in packs[e])
    assert all(p[0] in (0, 1, 3) for p in packs[0]) and all(p[0] == 2 for p in packs[2])
    good = [_frame_elems(40 + i, [packs[e][i] for e in range(3)]) for i in range(12)]
    bad = {}
    # 1: element 1's length reaches past the record (its length word is at byte 16 + n0)
    r = good[1]
    bad[1] = ("element 1 too long", _refresh_crc(_put32(r, 16 + len(packs[0][1]), len(r))), [0, -2, -2])
    # 3: the record ends inside element 2's length word: element 1 carries trailing bytes (no decoder looks at them) up to a
    # multiple of 8, the last four of which hold the record's CRC
    n0, n1 = len(packs[0][3]), len(packs[1][3])
    pad = 4 + (-(20 + n0 + n1 + 4)) % 8
    size = 20 + n0 + n1 + pad
    assert size % 8 == 0 and n1 + pad != std
    bad[3] = ("ends in element 2's length word", _frame_elems(43, [packs[0][3], packs[1][3] + b"\0" * pad], size=size), [0, 0, -2])
    assert struct.unpack_from("<i", bad[3][1], 0)[0] == len(bad[3][1]) == size
    # 5: the FLOAT element names an integer codec; 7: the INT element names the GF_CODEC_NONE slot
    r = good[5]
    at = 16 + len(packs[0][5]) + 4 + len(packs[1][5]) + 4
    assert r[at] == 2
    bad[5] = ("float names an integer codec", _refresh_crc(r[:at] + b"\x00" + r[at + 1:]), [0, 0, -1])
    r = good[7]
    bad[7] = ("int names the NONE slot", _refresh_crc(r[:16] + b"\x02" + r[17:]), [-1, 0, 0])
    # 9: a flipped payload bit (the checksum is what notices); 10: the type byte
    bad[9] = ("flipped payload bit", _flip(good[9], 16 + len(packs[0][9]) + 4 + 5, 3), [-1, -1, -1])
    r = good[10]
    bad[10] = ("type byte 3", _refresh_crc(r[:4] + b"\x03" + r[5:]), [-1, -1, -1])
    return dict(master=master, good=good, bad=bad, src=(s, c, f))


def _check_good(vals, st, idx, src, rows, tiles):
    """records `rows` of the answer hold tiles `tiles` of the sources, untouched by their neighbours"""
    s, c, f = src
    rows, tiles = list(rows), list(tiles)
    assert (st[:, rows] == 0).all() and list(idx[rows]) == [40 + t for t in tiles]
    assert np.array_equal(vals[0][rows], s[tiles])
    assert np.array_equal(_bits(vals[1][rows]), _bits(_icf_expect(c[tiles], ICF3)))
    assert np.array_equal(_bits(vals[2][rows]), _bits(f[tiles]))


@pytest.fixture(scope="module")
def damage5_batch(damage5):
    batch = [damage5["bad"][i][1] if i in damage5["bad"] else rec for i, rec in enumerate(damage5["good"])]
    blob, offsets = _shifted(batch, seed=21)
    return blob, offsets, damage5["master"].record_blob_elems_dev(R5, C5, blob, offsets, ELEMS5, verify_checksums=True)


def test_damaged_records(damage5, damage5_batch):
    bad, src = damage5["bad"], damage5["src"]
    blob, offsets, (idx, vals, st) = damage5_batch
    for i, (what, _, want) in bad.items():
        assert list(st[:, i]) == want, (what, st[:, i].tolist())
    keep = [i for i in range(12) if i not in bad]
    _check_good(vals, st, idx, src, keep, keep)
    # the elements in front of a failing one are decoded and keep their values
    s, c, f = src
    assert np.array_equal(vals[0][1], s[1]) and np.array_equal(vals[0][3], s[3]) and np.array_equal(vals[0][5], s[5])
    assert np.array_equal(_bits(vals[1][3]), _bits(_icf_expect(c[3], ICF3))) and np.array_equal(_bits(vals[1][5]), _bits(_icf_expect(c[5], ICF3)))
    assert np.array_equal(_bits(vals[1][7]), _bits(_icf_expect(c[7], ICF3))) and np.array_equal(_bits(vals[2][7]), _bits(f[7]))
    assert idx[1] == 41 and idx[9] == 49 and idx[10] == -1
    # without verification the flipped bit is the decoder's business, and only element 1's (where it lies)
    idx2, vals2, st2 = damage5["master"].record_blob_elems_dev(R5, C5, blob, offsets, ELEMS5, verify_checksums=False)
    assert st2[0, 9] == 0 and st2[2, 9] == 0 and np.array_equal(vals2[0][9], s[9]) and np.array_equal(_bits(vals2[2][9]), _bits(f[9]))
    for i, (what, _, want) in bad.items():
        if i != 9:
            assert list(st2[:, i]) == want, (what, st2[:, i].tolist())
    _check_good(vals2, st2, idx2, src, keep, keep)


def test_bad_offsets_are_bounds_errors_on_every_element(damage5):
    good, src = damage5["good"], damage5["src"]
    blob, offsets = _concat(good[:6])
    a = offsets.copy()
    a[1], a[2] = offsets[2], offsets[1]            # record 1 runs backwards; record 0 spans two records, record 2 starts at record 1's bytes
    idx, vals, st = damage5["master"].record_blob_elems_dev(R5, C5, blob, a, ELEMS5, verify_checksums=True)
    assert st[:, 1].tolist() == [-2, -2, -2] and idx[1] == -1
    _check_good(vals, st, idx, src, [0, 2, 3, 4, 5], [0, 1, 3, 4, 5])
    b = offsets.copy()
    b[-1] += 8                                     # the last record ends behind blob_bytes
    idx, vals, st = damage5["master"].record_blob_elems_dev(R5, C5, blob, b, ELEMS5, verify_checksums=True)
    assert st[:, 5].tolist() == [-2, -2, -2] and idx[5] == -1
    _check_good(vals, st, idx, src, range(5), range(5))


# ---------------------------------------------------------------- 6. the host form

def _same(host, dev):
    hi, hv, hs = host
    di, dv, ds = dev
    assert np.array_equal(hs, ds), (hs.tolist(), ds.tolist())
    assert np.array_equal(hi, di)
    for e in range(len(dv)):
        ok = ds[e] == 0
        assert hv[e].dtype == dv[e].dtype
        assert np.array_equal(hv[e][ok].view(np.uint8), dv[e][ok].view(np.uint8)), e


@pytest.mark.parametrize("nr,nc", SHAPES3)
def test_host_form_three_elements(three, nr, nc):
    t = three[(nr, nc)]
    _same(t["master"].record_blob_elems(nr, nc, t["blob"], t["offsets"], ELEMS3, verify_checksums=True), t["got"])


def test_host_form_damaged_records(damage5, damage5_batch):
    blob, offsets, got = damage5_batch
    _same(damage5["master"].record_blob_elems(R5, C5, blob, offsets, ELEMS5, verify_checksums=True), got)
